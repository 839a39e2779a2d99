// pm_flowseqwalk.h -- the walk of a flow ordered rule (include/pm_hip.h, "flow
// ordered rules"; DESIGN.md §4, "Flow ordered rules"): a chain's advance from
// its carried word over this call's occurrences, and a rule's evaluation over
// its chains.  One function for the device and the host: the kernel
// (pm_flowseqrules.hip, fs_eval_kernel) calls it with the frozen table, a host
// program (tests/sanitize/flow_seq_rules_check.cpp) with plain arrays, so that
// what is checked on the host is the code the device runs.
//
// The tables come through an accessor T:
//   uint32_t term(q), gap(q), len(q)   record q: gid | flags, d, L
//   bool range(q, a, b)    the sorted positions of record q's gid in this
//                          stream and call are occ(a) .. occ(b - 1), a <= b;
//                          false where the stream lacks the gid in this call
//   uint64_t occ(i)        for a <= i < b only; buffer positions
//   int64_t delta()        pos_in - the stream's offset: a buffer position p
//                          is the flow position p + delta()
//   bool carried(q)        the flow's row has the bit of record q's gid
//   uint64_t word(c)       chain word c of the flow's row
//   void store(c, w)       ... written (the commit)
// A rule's records are its positive terms in listed order, then the negated
// ones (pm_seqrules.h): a chain is a free record and the followers behind it.
//
// A chain word is 0 (the head is not yet seen) or (E + 1) << 6 | k: k the
// deepest level chosen so far, E the flow byte at which its occurrence ends.
// Greedy is exact across calls: E_i depends only on the occurrences at or
// below it, and a later call only adds larger positions, so a level once
// chosen never changes and the next level is the first occurrence at or above
// E + d + L among this call's -- an earlier call held none, or it had chosen.
//
// Memory safety does not depend on the data: a level is clamped to the
// chain's last, the loop over the levels to 64 turns, a bisection stays
// inside the range the accessor gave, and the accessor tests a chain-word
// index itself.
#ifndef PM_FLOWSEQWALK_H
#define PM_FLOWSEQWALK_H

#include <cstdint>

#if defined(__HIPCC__)
#define PM_FSW_HD __host__ __device__ __forceinline__
#else
#define PM_FSW_HD inline
#endif

constexpr uint32_t PM_FSW_FREE = 0xFFFFFFFFu;   // PM_SEQ_FREE
constexpr uint32_t PM_FSW_NEGATED = 1u << 31;  // PM_RULE_NEGATED
constexpr uint32_t PM_FSW_LEVEL_MASK = 63;

// The chain of records [q0, q1), 2 <= q1 - q0 <= 64, from its carried word:
// the word after this call's occurrences.  completed: the chain's last level
// was chosen in this call, at buffer position cpos.
template <class T>
PM_FSW_HD uint64_t pm_fsw_advance(const T& t, uint32_t q0, uint32_t q1, uint64_t word, bool& completed,
                                  uint64_t& cpos) {
    completed = false;
    const uint32_t last = (q1 - q0 - 1) & PM_FSW_LEVEL_MASK;
    const int64_t delta = t.delta();
    uint32_t k = 0;
    uint64_t e = 0;  // flow coordinates
    if (word == 0) {
        uint64_t a = 0, b = 0;
        if (!t.range(q0, a, b) || a >= b) return 0;
        const uint64_t p = t.occ(a);  // the head at its first position
        e = (uint64_t)((int64_t)p + delta);
        if (last == 0) {
            completed = true;
            cpos = p;
        }
    } else {
        k = (uint32_t)(word & PM_FSW_LEVEL_MASK);
        k = k < last ? k : last;
        e = (word >> 6) - 1;
    }
    for (uint32_t turn = 0; turn < 64 && k < last; ++turn) {
        const uint32_t q = q0 + k + 1;
        // the follower begins at least d bytes after level k has ended: it ends at or above e + d + L
        const int64_t need_flow = (int64_t)(e + (uint64_t)t.gap(q) + (uint64_t)t.len(q));
        const int64_t need_buf = need_flow - delta;
        const uint64_t need = need_buf < 0 ? 0 : (uint64_t)need_buf;  // at or before the first byte: the range's first
        uint64_t lo = 0, end = 0;
        if (!t.range(q, lo, end)) break;
        uint64_t hi = end;
        while (lo < hi) {  // at most 64 turns
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (t.occ(mid) < need) lo = mid + 1;
            else hi = mid;
        }
        if (lo >= end) break;
        const uint64_t p = t.occ(lo);
        e = (uint64_t)((int64_t)p + delta);
        ++k;
        if (k == last) {
            completed = true;
            cpos = p;
        }
    }
    return ((e + 1) << 6) | k;
}

// A whole rule, records [t0, t1), t1 - t0 <= 64, chain words [c0, c1): whether
// it fires in this call -- every chain done, at least one of them completed in
// this call, no negated gid carried or held -- and hp, the largest completing
// position of this call.  COMMIT: every chain is advanced whatever the
// outcome and a word that changed is stored; without it the walk stops at the
// first failure.
template <bool COMMIT, class T>
PM_FSW_HD bool pm_fsw_rule(T& t, uint32_t t0, uint32_t t1, uint32_t c0, uint32_t c1, uint64_t& hp) {
    hp = 0;
    bool fires = true, fresh = false;
    uint32_t c = c0, q = t0;
    while (q < t1) {  // every turn takes at least one record
        if (!COMMIT && !fires) return false;
        uint64_t a = 0, b = 0;
        if (t.term(q) & PM_FSW_NEGATED) {
            if (t.carried(q) || t.range(q, a, b)) fires = false;
            ++q;
            continue;
        }
        uint32_t e = q + 1;
        while (e < t1 && !(t.term(e) & PM_FSW_NEGATED) && t.gap(e) != PM_FSW_FREE) ++e;
        if (e - q == 1) {  // a chain of one term: a bit
            if (!t.carried(q)) {
                if (t.range(q, a, b) && a < b) {
                    const uint64_t p = t.occ(a);
                    fresh = true;
                    hp = p > hp ? p : hp;
                } else {
                    fires = false;
                }
            }
        } else if (c >= c1) {
            fires = false;
        } else {
            const uint64_t w = t.word(c);
            bool completed = false;
            uint64_t cpos = 0;
            const uint64_t nw = pm_fsw_advance(t, q, e, w, completed, cpos);
            if (completed) {
                fresh = true;
                hp = cpos > hp ? cpos : hp;
            }
            if (nw == 0 || (uint32_t)(nw & PM_FSW_LEVEL_MASK) != ((e - q - 1) & PM_FSW_LEVEL_MASK)) fires = false;
            if (COMMIT && nw != w) t.store(c, nw);
            ++c;
        }
        q = e;
    }
    return fires && fresh;
}

#endif  // PM_FLOWSEQWALK_H
