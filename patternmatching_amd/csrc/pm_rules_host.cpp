// pm_rules_host.cpp -- the host side of the rules (include/pm_hip.h,
// "rules"): the checks and the inverted index of a rule set, the host twin of
// the device call and the scratch formula.  Plain C++: no handle, no device,
// no HIP.
#include <algorithm>
#include <utility>
#include <vector>

#include "pm_hip.h"
#include "pm_rules.h"

extern "C" size_t pm_hip_rules_scratch_bytes(uint64_t cap, int64_t nseg) {
    if (cap > PM_BS_MAX_CAP || nseg < 0 || nseg >= PM_BS_MAX_NSEG) return (size_t)-1;
    return pm_rules_layout(cap, nseg).bytes;
}

namespace {

constexpr uint32_t GID_MASK = (uint32_t)PM_BS_GID_MASK;

// The checks of a rule set that need no dictionary: the CSR's shape, 1 to 64
// terms per rule, no unknown bits, a positive term, no gid twice, at most one
// PM_RULE_FAST and never on a negated term.
bool rules_well_formed(const uint32_t* term_ptr, const uint32_t* terms, size_t nrules) {
    if (!term_ptr || !terms || nrules == 0 || nrules > PM_RL_MAX_RULES || term_ptr[0] != 0) return false;
    for (size_t r = 0; r < nrules; ++r) {
        const uint32_t a = term_ptr[r], b = term_ptr[r + 1];
        if (b <= a || b - a > PM_RL_MAX_TERMS) return false;
        uint32_t positive = 0, fast = 0;
        for (uint32_t k = a; k < b; ++k) {
            const uint32_t t = terms[k];
            if (t & ~(GID_MASK | PM_RL_NEGATED | PM_RL_FAST)) return false;
            if ((t & PM_RL_FAST) && ((t & PM_RL_NEGATED) || fast++)) return false;
            if (!(t & PM_RL_NEGATED)) ++positive;
            for (uint32_t q = a; q < k; ++q)
                if (((terms[q] ^ t) & GID_MASK) == 0) return false;
        }
        if (!positive) return false;
    }
    return true;
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

struct Key {
    uint64_t stream, gid, pos;
    bool operator<(const Key& o) const {
        return stream != o.stream ? stream < o.stream : gid != o.gid ? gid < o.gid : pos < o.pos;
    }
};

// The position of gid in the stream's set [lo, hi) (ascending by gid), or false.
bool in_set(const Key* lo, const Key* hi, uint64_t gid, uint64_t& pos) {
    const Key* it = std::lower_bound(lo, hi, gid, [](const Key& k, uint64_t g) { return k.gid < g; });
    if (it == hi || it->gid != gid) return false;
    pos = it->pos;
    return true;
}

}  // namespace

extern "C" int pm_flat_rule_tables(const uint32_t* term_ptr, const uint32_t* terms, size_t nrules,
                                   const uint32_t* pattern_len, size_t npat, uint32_t* anchor_ptr_out,
                                   uint32_t* anchor_rules_out, uint32_t* anchor_term_out) {
    if (!pattern_len || npat >= ((size_t)1 << PM_BS_GID_BITS) || !anchor_ptr_out || !anchor_rules_out ||
        !anchor_term_out || !rules_well_formed(term_ptr, terms, nrules))
        return -2;
    std::vector<uint32_t> anchor(nrules);  // the index in terms of each rule's anchor
    for (size_t r = 0; r < nrules; ++r) {
        uint32_t best = UINT32_MAX;
        bool fast = false;
        for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k) {
            const uint32_t t = terms[k], g = t & GID_MASK;
            if (g > npat || pattern_len[g] == 0) return -2;
            if ((t & PM_RL_NEGATED) || fast) continue;
            if (t & PM_RL_FAST) {
                best = k;
                fast = true;
                continue;
            }
            const uint32_t bg = best == UINT32_MAX ? 0 : terms[best] & GID_MASK;
            if (best == UINT32_MAX || pattern_len[g] > pattern_len[bg] || (pattern_len[g] == pattern_len[bg] && g < bg))
                best = k;
        }
        anchor[r] = best;
    }
    // nothing was written so far; the index by counting
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

int pm_rules_image(const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, const uint32_t* pattern_len,
                   size_t npat, PmRulesImage& img) {
    if (!rules_well_formed(term_ptr, terms, nrules)) return -2;
    img.anchor_ptr.assign(npat + 2, 0);
    img.anchor_rules.assign(nrules, 0);
    std::vector<uint32_t> anchor(nrules);
    if (pm_flat_rule_tables(term_ptr, terms, nrules, pattern_len, npat, img.anchor_ptr.data(), img.anchor_rules.data(),
                            anchor.data()))
        return -2;
    img.rterm_ptr.assign(nrules + 1, 0);
    img.rterms.clear();
    img.rterms.reserve(term_ptr[nrules] - nrules + 1);
    img.min_len = UINT32_MAX;
    for (size_t r = 0; r < nrules; ++r) {
        for (uint32_t neg = 0; neg < 2; ++neg)
            for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k) {
                const uint32_t t = terms[k];
                if (!neg) img.min_len = std::min(img.min_len, pattern_len[t & GID_MASK]);
                if (k != anchor[r] && ((t & PM_RL_NEGATED) != 0) == (neg != 0))
                    img.rterms.push_back(t & (GID_MASK | PM_RL_NEGATED));
            }
        img.rterm_ptr[r + 1] = (uint32_t)img.rterms.size();
    }
    if (img.rterms.empty()) img.rterms.push_back(0);  // never read: every range is empty
    return 0;
}

extern "C" int pm_flat_rules_by_stream(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                                       const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, uint64_t* hits,
                                       size_t hits_cap, int64_t* rule_ptr) {
    if ((nevents && !events) || (nseg && (!offsets || !rule_ptr)) || (hits_cap && !hits) ||
        nseg >= (size_t)PM_BS_MAX_NSEG || nevents > PM_BS_MAX_CAP || (hits && hits == events) ||
        !rules_well_formed(term_ptr, terms, nrules))
        return -2;
    if (nseg == 0) return 0;
    // the sets: one key per (stream, gid), at its smallest position, ascending by stream then gid
    std::vector<Key> keys;
    keys.reserve(nevents);
    for (size_t k = 0; k < nevents; ++k) {
        const uint64_t ev = events[k];
        const int64_t j = stream_of(offsets, nseg, (int64_t)(ev >> PM_BS_GID_BITS));
        if (j >= 0) keys.push_back({(uint64_t)j, ev & PM_BS_GID_MASK, ev >> PM_BS_GID_BITS});
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end(),
                           [](const Key& a, const Key& b) { return a.stream == b.stream && a.gid == b.gid; }),
               keys.end());
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
        while (at < keys.size() && keys[at].stream == j) ++at;
        const Key *klo = keys.data() + lo, *khi = keys.data() + at;
        mine.clear();
        for (const Key* k = klo; k < khi; ++k) {
            auto it = std::lower_bound(by_first.begin(), by_first.end(), std::make_pair((uint32_t)k->gid, 0u));
            for (; it != by_first.end() && it->first == k->gid; ++it) {
                const uint32_t r = it->second;
                uint64_t position = 0;
                bool fires = true;
                for (uint32_t q = term_ptr[r]; fires && q < term_ptr[r + 1]; ++q) {
                    uint64_t p = 0;
                    const bool held = in_set(klo, khi, terms[q] & GID_MASK, p);
                    if (terms[q] & PM_RL_NEGATED) fires = !held;
                    else if (held) position = std::max(position, p);
                    else fires = false;
                }
                if (fires) mine.push_back((position << PM_BS_GID_BITS) | r);
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
