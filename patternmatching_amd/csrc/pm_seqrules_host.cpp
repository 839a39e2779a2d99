// pm_seqrules_host.cpp -- the host side of the ordered rules (include/pm_hip.h,
// "ordered rules"): the checks, the anchors and the device image of a rule
// set, the host twin of the device call and the scratch formula.  Plain C++:
// no handle, no device, no HIP.
#include <algorithm>
#include <utility>
#include <vector>

#include "pm_hip.h"
#include "pm_seqrules.h"

extern "C" size_t pm_hip_seq_rules_scratch_bytes(uint64_t cap, int64_t nseg) {
    if (cap > PM_BS_MAX_CAP || nseg < 0 || nseg >= PM_BS_MAX_NSEG) return (size_t)-1;
    return pm_seq_rules_layout(cap, nseg).bytes;
}

namespace {

constexpr uint32_t GID_MASK = (uint32_t)PM_BS_GID_MASK;

// The checks of an ordered rule set: pm_hip_set_rules' (the CSR's shape, 1 to
// 64 terms per rule, no unknown bits, a positive term, at most one
// PM_RULE_FAST and never on a negated term, every gid a pattern's) and the
// gaps': PM_SEQ_FREE or at most 0x7FFFFFFF, free on a negated term and on the
// first positive one.  A gid may come again among the positive terms, each
// time after the first as a following term; never both positive and negated.
// The withins' (NULL: every one free): PM_SEQ_FREE, or on a following term a
// bound of at most 0x7FFFFFFF and of at least d + L, below which no occurrence
// can meet the link.
bool seq_well_formed(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps, size_t nrules,
                     const uint32_t* pattern_len, size_t npat, const uint32_t* withins = nullptr) {
    if (!term_ptr || !terms || !gaps || !pattern_len || npat >= ((size_t)1 << PM_BS_GID_BITS) || nrules == 0 ||
        nrules > PM_RL_MAX_RULES || term_ptr[0] != 0)
        return false;
    for (size_t r = 0; r < nrules; ++r) {
        const uint32_t a = term_ptr[r], b = term_ptr[r + 1];
        if (b <= a || b - a > PM_RL_MAX_TERMS) return false;
        uint32_t positive = 0, fast = 0;
        for (uint32_t k = a; k < b; ++k) {
            const uint32_t t = terms[k], g = t & GID_MASK, gap = gaps[k];
            if (t & ~(GID_MASK | PM_RL_NEGATED | PM_RL_FAST)) return false;
            if ((t & PM_RL_FAST) && ((t & PM_RL_NEGATED) || fast++)) return false;
            if (g > npat || pattern_len[g] == 0) return false;
            if (gap != PM_SQ_FREE && (gap > PM_SQ_MAX_GAP || (t & PM_RL_NEGATED) || positive == 0)) return false;
            const uint32_t w = withins ? withins[k] : PM_SQ_FREE;
            if (w != PM_SQ_FREE &&
                (gap == PM_SQ_FREE || w > PM_SQ_MAX_GAP || (uint64_t)w < (uint64_t)gap + pattern_len[g]))
                return false;
            if (!(t & PM_RL_NEGATED)) ++positive;
            for (uint32_t q = a; q < k; ++q)
                if (((terms[q] ^ t) & GID_MASK) == 0 && (((terms[q] | t) & PM_RL_NEGATED) || gap == PM_SQ_FREE))
                    return false;
        }
        if (!positive) return false;
    }
    return true;
}

// Each rule's anchor, as an index into terms: the PM_RULE_FAST term, else the
// positive term with the longest pattern, ties going to the smaller gid and
// then to the term listed first.
void pick_anchors(const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, const uint32_t* pattern_len,
                  std::vector<uint32_t>& anchor) {
    anchor.assign(nrules, 0);
    for (size_t r = 0; r < nrules; ++r) {
        uint32_t best = UINT32_MAX;
        for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k) {
            const uint32_t t = terms[k], g = t & GID_MASK;
            if (t & PM_RL_NEGATED) continue;
            if (t & PM_RL_FAST) {
                best = k;
                break;
            }
            const uint32_t bg = best == UINT32_MAX ? 0 : terms[best] & GID_MASK;
            if (best == UINT32_MAX || pattern_len[g] > pattern_len[bg] || (pattern_len[g] == pattern_len[bg] && g < bg))
                best = k;
        }
        anchor[r] = best;
    }
}

// The stream of position p, or -1 (pm_bystream_host.cpp's bisection).
int64_t stream_of(const int64_t* offs, size_t nseg, int64_t p) {
    size_t lo = 0, hi = nseg + 1;
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (offs[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0 || lo > nseg) return -1;
    const size_t j = lo - 1;
    return offs[j] <= p && p < offs[j + 1] ? (int64_t)j : -1;
}

struct Occ {
    uint64_t stream, gid, pos;
    bool operator<(const Occ& o) const {
        return stream != o.stream ? stream < o.stream : gid != o.gid ? gid < o.gid : pos < o.pos;
    }
};

// The occurrences of gid in the stream's part [lo, hi) of the index (ascending
// by gid, then position): [first, last), empty where the stream lacks it.
std::pair<const Occ*, const Occ*> occ_of(const Occ* lo, const Occ* hi, uint64_t gid) {
    const Occ* a = std::lower_bound(lo, hi, gid, [](const Occ& k, uint64_t g) { return k.gid < g; });
    const Occ* b = std::upper_bound(a, hi, gid, [](uint64_t g, const Occ& k) { return g < k.gid; });
    return {a, b};
}

}  // namespace

extern "C" int pm_flat_seq_rule_tables(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                                       size_t nrules, const uint32_t* pattern_len, size_t npat,
                                       uint32_t* anchor_ptr_out, uint32_t* anchor_rules_out,
                                       uint32_t* anchor_term_out) {
    return pm_flat_seq_rule_tables_within(term_ptr, terms, gaps, nullptr, nrules, pattern_len, npat, anchor_ptr_out,
                                          anchor_rules_out, anchor_term_out);
}

// The bounds choose no anchor: the tables are pm_flat_seq_rule_tables'.
extern "C" int pm_flat_seq_rule_tables_within(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                                              const uint32_t* withins, size_t nrules, const uint32_t* pattern_len,
                                              size_t npat, uint32_t* anchor_ptr_out, uint32_t* anchor_rules_out,
                                              uint32_t* anchor_term_out) {
    if (!anchor_ptr_out || !anchor_rules_out || !anchor_term_out ||
        !seq_well_formed(term_ptr, terms, gaps, nrules, pattern_len, npat, withins))
        return -2;
    std::vector<uint32_t> anchor;
    pick_anchors(term_ptr, terms, nrules, pattern_len, anchor);
    std::fill(anchor_ptr_out, anchor_ptr_out + npat + 2, 0u);
    for (size_t r = 0; r < nrules; ++r) ++anchor_ptr_out[(terms[anchor[r]] & GID_MASK) + 1];
    for (size_t g = 0; g <= npat; ++g) anchor_ptr_out[g + 1] += anchor_ptr_out[g];
    std::vector<uint32_t> at(anchor_ptr_out, anchor_ptr_out + npat + 1);
    for (size_t r = 0; r < nrules; ++r) {  // ascending rule indices inside a gid's range
        anchor_rules_out[at[terms[anchor[r]] & GID_MASK]++] = (uint32_t)r;
        anchor_term_out[r] = anchor[r];
    }
    return 0;
}

int pm_seq_rules_image(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps, size_t nrules,
                       const uint32_t* pattern_len, size_t npat, PmSeqRulesImage& img) {
    return pm_seq_rules_image_within(term_ptr, terms, gaps, nullptr, nrules, pattern_len, npat, img);
}

int pm_seq_rules_image_within(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                              const uint32_t* withins, size_t nrules, const uint32_t* pattern_len, size_t npat,
                              PmSeqRulesImage& img) {
    if (!seq_well_formed(term_ptr, terms, gaps, nrules, pattern_len, npat, withins)) return -2;
    img.anchor_ptr.assign(npat + 2, 0);
    img.anchor_rules.assign(nrules, 0);
    std::vector<uint32_t> anchor(nrules);
    if (pm_flat_seq_rule_tables(term_ptr, terms, gaps, nrules, pattern_len, npat, img.anchor_ptr.data(),
                                img.anchor_rules.data(), anchor.data()))
        return -2;
    img.rterm_ptr.assign(nrules + 1, 0);
    img.recs.clear();
    img.recs.reserve((size_t)term_ptr[nrules] * PM_SQ_REC);
    img.wins.clear();
    img.within_run = 0;
    img.min_len = UINT32_MAX;
    for (size_t r = 0; r < nrules; ++r) {
        uint32_t run = 0;  // counted over the records, where a rule's positive terms are consecutive
        for (uint32_t neg = 0; neg < 2; ++neg)
            for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k) {
                const uint32_t t = terms[k], len = pattern_len[t & GID_MASK];
                if (((t & PM_RL_NEGATED) != 0) != (neg != 0)) continue;
                img.min_len = std::min(img.min_len, len);
                img.recs.push_back(t & (GID_MASK | PM_RL_NEGATED));
                img.recs.push_back(gaps[k]);
                img.recs.push_back(len);
                const uint32_t w = withins ? withins[k] : PM_SQ_FREE;
                img.wins.push_back(w);
                run = w != PM_SQ_FREE ? run + 1 : 0;
                img.within_run = std::max(img.within_run, run);
            }
        img.rterm_ptr[r + 1] = (uint32_t)(img.recs.size() / PM_SQ_REC);
    }
    if (!img.within_run) img.wins.clear();
    return 0;
}


namespace {

// What the twins share: the checks, the index, the rules by the gid of their
// first positive term, and the output.  eval(klo, khi, r, position) says
// whether rule r fires over the stream's part [klo, khi) of the index, and
// where.
template <class Eval>
int by_stream(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg, const uint32_t* term_ptr,
              const uint32_t* terms, const uint32_t* gaps, const uint32_t* withins, size_t nrules,
              const uint32_t* pattern_len, size_t npat, uint64_t* hits, size_t hits_cap, int64_t* rule_ptr, Eval eval) {
    if ((nevents && !events) || (nseg && (!offsets || !rule_ptr)) || (hits_cap && !hits) ||
        nseg >= (size_t)PM_BS_MAX_NSEG || nevents > PM_BS_MAX_CAP || (hits && hits == events) ||
        !seq_well_formed(term_ptr, terms, gaps, nrules, pattern_len, npat, withins))
        return -2;
    if (nseg == 0) return 0;
    // the index: every event inside a stream, ascending by stream, gid and position
    std::vector<Occ> occ;
    occ.reserve(nevents);
    for (size_t k = 0; k < nevents; ++k) {
        const uint64_t ev = events[k];
        const int64_t j = stream_of(offsets, nseg, (int64_t)(ev >> PM_BS_GID_BITS));
        if (j >= 0) occ.push_back({(uint64_t)j, ev & PM_BS_GID_MASK, ev >> PM_BS_GID_BITS});
    }
    std::sort(occ.begin(), occ.end());
    // the rules by the gid of their first positive term: a rule is looked at
    // only in a stream that holds that term
    std::vector<std::pair<uint32_t, uint32_t>> by_first(nrules);
    for (size_t r = 0; r < nrules; ++r) {
        uint32_t k = term_ptr[r];
        while (terms[k] & PM_RL_NEGATED) ++k;  // well formed: there is one
        by_first[r] = {terms[k] & GID_MASK, (uint32_t)r};
    }
    std::sort(by_first.begin(), by_first.end());
    size_t total = 0, at = 0;
    std::vector<uint64_t> mine;
    for (size_t j = 0; j < nseg; ++j) {
        rule_ptr[j] = (int64_t)total;
        const size_t lo = at;
        while (at < occ.size() && occ[at].stream == j) ++at;
        const Occ *klo = occ.data() + lo, *khi = occ.data() + at;
        mine.clear();
        for (const Occ* k = klo; k < khi; ++k) {
            if (k > klo && k[-1].gid == k->gid) continue;  // each gid of the stream once
            auto it = std::lower_bound(by_first.begin(), by_first.end(), std::make_pair((uint32_t)k->gid, 0u));
            for (; it != by_first.end() && it->first == k->gid; ++it) {
                const uint32_t r = it->second;
                uint64_t position = 0;
                if (eval(klo, khi, r, position)) mine.push_back((position << PM_BS_GID_BITS) | r);
            }
        }
        std::sort(mine.begin(), mine.end());
        for (const uint64_t h : mine) {
            if (total < hits_cap) hits[total] = h;
            ++total;
        }
    }
    rule_ptr[nseg] = (int64_t)total;
    return 0;
}

}  // namespace

// Greedy: a chain's head at its first position, each follower at its first
// position that satisfies the link.
extern "C" int pm_flat_seq_rules_by_stream(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                                           const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                                           size_t nrules, const uint32_t* pattern_len, size_t npat, uint64_t* hits,
                                           size_t hits_cap, int64_t* rule_ptr) {
    return by_stream(events, nevents, offsets, nseg, term_ptr, terms, gaps, nullptr, nrules, pattern_len, npat, hits,
                     hits_cap, rule_ptr, [&](const Occ* klo, const Occ* khi, uint32_t r, uint64_t& position) {
                         uint64_t prev = 0;
                         bool fires = true;
                         for (uint32_t q = term_ptr[r]; fires && q < term_ptr[r + 1]; ++q) {
                             const uint32_t t = terms[q], g = t & GID_MASK;
                             const auto range = occ_of(klo, khi, g);
                             if (t & PM_RL_NEGATED) {
                                 fires = range.first == range.second;
                                 continue;
                             }
                             const Occ* o = range.first;
                             if (gaps[q] != PM_SQ_FREE) {  // the first occurrence that begins gap bytes after prev or later
                                 const uint64_t need = prev + gaps[q] + pattern_len[g];
                                 o = std::lower_bound(range.first, range.second, need,
                                                      [](const Occ& k2, uint64_t p) { return k2.pos < p; });
                             }
                             if (o == range.second) {
                                 fires = false;
                                 continue;
                             }
                             prev = o->pos;
                             position = std::max(position, prev);
                         }
                         return fires;
                     });
}

// The feasible sets, level by level, and not the device's walk: an occurrence
// o of a following term is feasible iff some feasible occurrence f of the
// level before has o - w <= f <= o - d - L.  The level before is sorted, so
// those f are a contiguous part of it -- two bisections -- and a prefix count
// of its feasible flags says whether one of them is feasible.  A chain's head
// is feasible everywhere.  The smallest feasible position of a level grows
// along a chain, so the largest of them over all levels is the largest over
// the chains' last levels: the hit's position.
extern "C" int pm_flat_seq_rules_by_stream_within(const uint64_t* events, size_t nevents, const int64_t* offsets,
                                                  size_t nseg, const uint32_t* term_ptr, const uint32_t* terms,
                                                  const uint32_t* gaps, const uint32_t* withins, size_t nrules,
                                                  const uint32_t* pattern_len, size_t npat, uint64_t* hits,
                                                  size_t hits_cap, int64_t* rule_ptr) {
    std::vector<uint64_t> before, level;  // the positions of the level before and of this one
    std::vector<uint32_t> count, flags;   // count[i]: the feasible ones among before[0, i)
    return by_stream(
        events, nevents, offsets, nseg, term_ptr, terms, gaps, withins, nrules, pattern_len, npat, hits, hits_cap,
        rule_ptr, [&](const Occ* klo, const Occ* khi, uint32_t r, uint64_t& position) {
            before.clear();
            count.assign(1, 0);
            for (uint32_t q = term_ptr[r]; q < term_ptr[r + 1]; ++q) {
                const uint32_t t = terms[q], g = t & GID_MASK;
                const auto range = occ_of(klo, khi, g);
                if (t & PM_RL_NEGATED) {
                    if (range.first != range.second) return false;
                    continue;
                }
                level.clear();
                for (const Occ* o = range.first; o < range.second; ++o) level.push_back(o->pos);
                flags.assign(level.size(), 1);
                if (gaps[q] != PM_SQ_FREE) {
                    const uint64_t dl = (uint64_t)gaps[q] + pattern_len[g];
                    const uint32_t w = withins ? withins[q] : PM_SQ_FREE;
                    for (size_t i = 0; i < level.size(); ++i) {
                        const uint64_t o = level[i];
                        size_t hi = 0, lo = 0;
                        if (o >= dl) hi = (size_t)(std::upper_bound(before.begin(), before.end(), o - dl) - before.begin());
                        if (w != PM_SQ_FREE && o > w)
                            lo = (size_t)(std::lower_bound(before.begin(), before.end(), o - w) - before.begin());
                        flags[i] = hi > lo && count[hi] > count[lo];
                    }
                }
                count.assign(level.size() + 1, 0);
                uint64_t first = 0;
                for (size_t i = 0; i < level.size(); ++i) {
                    if (flags[i] && !count[i]) first = level[i];
                    count[i + 1] = count[i] + flags[i];
                }
                if (!count[level.size()]) return false;
                position = std::max(position, first);
                before.swap(level);
            }
            return true;
        });
}
