// pm_seqwalk.h -- the exact walk of an ordered rule whose links may carry an
// upper bound (include/pm_hip.h, "ordered rules", within; DESIGN.md §4, "The
// walk with an upper bound").  One function for the device and the host: the
// kernel (pm_seqrules.hip, sq_eval_within_kernel) calls it with cursors in
// LDS, a host program (tests/sanitize/within_rules_check.cpp) with a plain
// array, so that what is checked on the host is the code the device runs.
//
// The tables come through an accessor T:
//   uint32_t term(q), gap(q), len(q), within(q)   record q: gid | flags, d, L, w
//   bool range(q, a, b)    the sorted positions of record q's gid in this
//                          stream are occ(a) .. occ(b - 1), a <= b; false
//                          where the stream lacks the gid
//   uint64_t occ(i)        for a <= i < b only
// A rule's records are its positive terms in listed order, then the negated
// ones (pm_seqrules.h).
//
// A chain is cut into runs of consecutive bounded links.  A run's head is a
// free term or the follower of an unbounded link; for the latter only E, the
// smallest feasible position of the level before, matters, and the head's
// feasible set is occ at or above lb = E + d + L.  Inside a run next(i, x) is
// the smallest feasible position of level i at or above x:
//   level 0:  a lower bound in the head's range, at max(x, lb);
//   level i:  c = the first position of level i at or above x (none: none);
//             q = next(i - 1, c - w_i) (none: none -- a later c asks for a
//             later predecessor still);  q + d_i + L_i <= c: the answer is c;
//             else x = q + d_i + L_i > c and again: no feasible predecessor
//             lies in [c - w_i, q), so no position below x is feasible.
// The run's value is next(top, 0).  The queries to a level never decrease, so
// a level keeps one cursor into its range and a bit that says that the
// position under the cursor is feasible; a query at or below such a position
// is answered at once.  Every other turn moves one cursor strictly forward or
// touches a level for the first time.
//
// The walk is written with a level index and no recursion.  Going down, x is
// the query; coming up, x is the answer of the level below, and the candidate
// that asked is the position under the level's cursor.  The cursors are u32
// offsets from the range's start, cursor of level i at curs[i * stride], the
// top level's in a register: a run of k links needs k cursors.
//
// Memory safety does not depend on the data: a cursor is clamped to its
// range's length before it is used, a range to 2^32 - 1 positions, a run to
// kmax links (the cursors the caller has), and the loop to max_turns.
#ifndef PM_SEQWALK_H
#define PM_SEQWALK_H

#include <cstdint>

#if defined(__HIPCC__)
#define PM_SW_HD __host__ __device__ __forceinline__
#else
#define PM_SW_HD inline
#endif

constexpr uint32_t PM_SW_FREE = 0xFFFFFFFFu;   // PM_SEQ_FREE
constexpr uint32_t PM_SW_NEGATED = 1u << 31;  // PM_RULE_NEGATED

// The first index in [cur, len) whose position is at or above x, or len:
// steps of 1, 2, 4, ... from the cursor, then a bisection between the last
// two probes.  At most 2 log2(len) + 2 loads.
template <class T>
PM_SW_HD uint64_t pm_sw_gallop(const T& t, uint64_t a, uint64_t cur, uint64_t len, uint64_t x) {
    if (cur >= len || t.occ(a + cur) >= x) return cur < len ? cur : len;
    uint64_t lo = cur, hi = len;  // occ(a + lo) < x
    for (uint64_t step = 1; step != 0; step <<= 1) {  // at most 64 turns
        const uint64_t at = lo + step;
        if (at >= len) break;
        if (t.occ(a + at) >= x) {
            hi = at;
            break;
        }
        lo = at;
    }
    ++lo;
    while (lo < hi) {  // at most 64 turns
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (t.occ(a + mid) < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One run: records q0 (the head) .. q0 + k, the links into q0 + 1 .. q0 + k
// bounded; k <= min(kmax, 63).  value = the smallest feasible position of the
// run's last level; false where there is none.
template <class T>
PM_SW_HD bool pm_sw_run(const T& t, uint32_t q0, uint32_t k, uint64_t lb, uint32_t* curs, uint32_t stride,
                        uint32_t kmax, uint64_t max_turns, uint64_t& value) {
    if (k > kmax || k > 63) return false;
    uint64_t verified = 0, touched = 0;  // a bit per level
    uint32_t topcur = 0;
    uint64_t top_a = 0, top_b = 0, low_a = 0, low_b = 0;
    uint32_t low_lvl = 0xFFFFFFFFu;
    bool top_have = false;
    uint32_t lvl = k;
    uint64_t x = 0;
    bool down = true;
    for (uint64_t turn = 0; turn < max_turns; ++turn) {
        const uint64_t bit = 1ull << lvl;
        // the level's range: the top level's is looked up once, the level last visited below it is remembered,
        // so that a run of one link -- the common one -- looks each of its two ranges up once
        uint64_t a = 0, b = 0;
        if (lvl == k) {
            if (!top_have) {
                if (!t.range(q0 + lvl, top_a, top_b)) return false;
                top_have = true;
            }
            a = top_a;
            b = top_b;
        } else if (lvl == low_lvl) {
            a = low_a;
            b = low_b;
        } else {
            if (!t.range(q0 + lvl, a, b)) return false;
            low_lvl = lvl;
            low_a = a;
            low_b = b;
        }
        uint64_t len = b - a;
        if (len > 0xFFFFFFFFull) len = 0xFFFFFFFFull;
        uint64_t cur = lvl == k ? topcur : (touched & bit) ? curs[(uint64_t)lvl * stride] : 0u;
        if (cur > len) cur = len;
        const uint64_t dl = lvl ? (uint64_t)t.gap(q0 + lvl) + t.len(q0 + lvl) : 0;
        if (!down) {  // x answers next(lvl - 1, c - w) for the candidate c under this level's cursor
            if (cur >= len) return false;
            const uint64_t c = t.occ(a + cur);
            if (x + dl <= c) {
                verified |= bit;
                if (lvl == k) {
                    value = c;
                    return true;
                }
                x = c;
                ++lvl;
                continue;
            }
            x += dl;  // > c: every position below it is infeasible
            down = true;
        }
        if (lvl == 0 && x < lb) x = lb;
        bool known = (verified & bit) && cur < len && t.occ(a + cur) >= x;
        if (!known) {
            cur = pm_sw_gallop(t, a, cur, len, x);
            if (lvl == k) topcur = (uint32_t)cur;
            else curs[(uint64_t)lvl * stride] = (uint32_t)cur;
            touched |= bit;
            verified &= ~bit;
            if (cur >= len) return false;
            if (lvl == 0) {  // every position of the head at or above lb is feasible
                verified |= bit;
                known = true;
            }
        }
        const uint64_t c = t.occ(a + cur);
        if (known) {
            if (lvl == k) {
                value = c;
                return true;
            }
            x = c;
            ++lvl;
            down = false;
            continue;
        }
        const uint64_t w = t.within(q0 + lvl);
        x = c > w ? c - w : 0;  // never below 0
        --lvl;
    }
    return false;
}

// A whole rule, records [t0, t1), t1 - t0 <= 64: whether it fires, and hp, the
// largest of the runs' values (positions grow along a chain, so a chain's last
// run has its largest).  The negated records come last.
template <class T>
PM_SW_HD bool pm_sw_rule(const T& t, uint32_t t0, uint32_t t1, uint32_t* curs, uint32_t stride, uint32_t kmax,
                         uint64_t max_turns, uint64_t& hp) {
    hp = 0;
    uint64_t e_prev = 0;
    uint32_t q = t0;
    while (q < t1) {  // every turn takes at least one record
        if (t.term(q) & PM_SW_NEGATED) {
            uint64_t a, b;
            if (t.range(q, a, b)) return false;
            ++q;
            continue;
        }
        const uint32_t gap = t.gap(q);
        const uint64_t lb = gap == PM_SW_FREE ? 0 : e_prev + gap + t.len(q);
        uint32_t e = q;
        while (e + 1 < t1 && !(t.term(e + 1) & PM_SW_NEGATED) && t.within(e + 1) != PM_SW_FREE) ++e;
        if (!pm_sw_run(t, q, e - q, lb, curs, stride, kmax, max_turns, e_prev)) return false;
        hp = e_prev > hp ? e_prev : hp;
        q = e + 1;
    }
    return true;
}

#endif  // PM_SEQWALK_H
