// pm_flowrules_host.cpp -- the host side of the flow rules (include/pm_hip.h,
// "flow rules"): the checks, the bit numbering and the device tables of a rule
// set, the host twin of the device call and the scratch formula.  Plain C++:
// no handle, no device, no HIP.
#include <algorithm>
#include <utility>
#include <vector>

#include "pm_flowrules.h"
#include "pm_hip.h"

extern "C" size_t pm_hip_flow_rules_scratch_bytes(uint64_t cap, int64_t nseg) {
    if (cap > PM_BS_MAX_CAP || nseg < 0 || nseg >= PM_BS_MAX_NSEG) return (size_t)-1;
    return pm_rules_layout(cap, nseg).bytes;
}

namespace {

constexpr uint32_t GID_MASK = (uint32_t)PM_BS_GID_MASK;

// pm_rules_host.cpp's checks of a rule set that need no dictionary: the CSR's
// shape, 1 to 64 terms per rule, no unknown bits, a positive term, no gid
// twice, at most one PM_RULE_FAST and never on a negated term.
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

// The distinct gids of every term, ascending: a gid's bit is its index here.
std::vector<uint32_t> term_gids(const uint32_t* term_ptr, const uint32_t* terms, size_t nrules) {
    std::vector<uint32_t> g(terms, terms + term_ptr[nrules]);
    for (uint32_t& t : g) t &= GID_MASK;
    std::sort(g.begin(), g.end());
    g.erase(std::unique(g.begin(), g.end()), g.end());
    return g;
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

struct New {
    uint64_t stream;
    uint32_t bit;
    uint64_t pos;
    bool operator<(const New& o) const {
        return stream != o.stream ? stream < o.stream : bit != o.bit ? bit < o.bit : pos < o.pos;
    }
};

}  // namespace

extern "C" int pm_flat_flow_rule_bits(const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, size_t npat,
                                      uint32_t* bit_by_gid_out, uint32_t* nbits_out) {
    if (npat >= ((size_t)1 << PM_BS_GID_BITS) || !bit_by_gid_out || !nbits_out ||
        !rules_well_formed(term_ptr, terms, nrules))
        return -2;
    const std::vector<uint32_t> gids = term_gids(term_ptr, terms, nrules);
    if (gids.front() == 0 || gids.back() > npat) return -2;
    std::fill(bit_by_gid_out, bit_by_gid_out + npat + 1, PM_FR_NO_BIT);
    for (size_t b = 0; b < gids.size(); ++b) bit_by_gid_out[gids[b]] = (uint32_t)b;
    *nbits_out = (uint32_t)gids.size();
    return 0;
}

int pm_flow_rules_image(const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, const uint32_t* pattern_len,
                        size_t npat, PmFlowRulesImage& img) {
    if (!pattern_len || npat >= ((size_t)1 << PM_BS_GID_BITS) || !rules_well_formed(term_ptr, terms, nrules)) return -2;
    for (uint32_t k = 0; k < term_ptr[nrules]; ++k) {
        const uint32_t g = terms[k] & GID_MASK;
        if (g > npat || pattern_len[g] == 0) return -2;
    }
    img.gid_bit.assign(npat + 1, PM_FR_NO_BIT);
    if (pm_flat_flow_rule_bits(term_ptr, terms, nrules, npat, img.gid_bit.data(), &img.nbits)) return -2;
    img.words = std::max(1u, (img.nbits + 63) / 64);
    // the index from every positive term's gid, by counting; ascending rules inside a gid's range
    img.idx_ptr.assign(npat + 2, 0);
    for (uint32_t k = 0; k < term_ptr[nrules]; ++k)
        if (!(terms[k] & PM_RL_NEGATED)) ++img.idx_ptr[(terms[k] & GID_MASK) + 1];
    img.max_fanout = *std::max_element(img.idx_ptr.begin(), img.idx_ptr.end());
    for (size_t g = 0; g <= npat; ++g) img.idx_ptr[g + 1] += img.idx_ptr[g];
    img.idx_rules.assign(img.idx_ptr[npat + 1], 0);
    std::vector<uint32_t> at(img.idx_ptr.begin(), img.idx_ptr.end() - 1);
    img.rterm_ptr.assign(nrules + 1, 0);
    img.rterms.clear();
    img.rterms.reserve(term_ptr[nrules]);
    img.min_len = UINT32_MAX;
    for (size_t r = 0; r < nrules; ++r) {
        // the first term: PM_RULE_FAST, else the longest positive pattern, ties to the smaller gid
        uint32_t first = UINT32_MAX;
        for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k) {
            const uint32_t t = terms[k], g = t & GID_MASK;
            img.min_len = std::min(img.min_len, pattern_len[g]);
            if (t & PM_RL_NEGATED) continue;
            img.idx_rules[at[g]++] = (uint32_t)r;
            if (first != UINT32_MAX && (terms[first] & PM_RL_FAST)) continue;
            const uint32_t fg = first == UINT32_MAX ? 0 : terms[first] & GID_MASK;
            if (first == UINT32_MAX || (t & PM_RL_FAST) || pattern_len[g] > pattern_len[fg] ||
                (pattern_len[g] == pattern_len[fg] && g < fg))
                first = k;
        }
        img.rterms.push_back(terms[first] & GID_MASK);
        for (uint32_t neg = 0; neg < 2; ++neg)
            for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k)
                if (k != first && ((terms[k] & PM_RL_NEGATED) != 0) == (neg != 0))
                    img.rterms.push_back(terms[k] & (GID_MASK | PM_RL_NEGATED));
        img.rterm_ptr[r + 1] = (uint32_t)img.rterms.size();
    }
    return 0;
}

// The prefix definition, stream by stream: C = the row's bits, N = the term
// gids the stream holds in this call that C lacks, each at its first position.
// A rule is looked at once per stream that holds one of its positive terms in N.
extern "C" int pm_flat_flow_rules(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                                  const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, uint64_t* sets,
                                  size_t nrows, size_t words, const int64_t* rows, uint32_t flags, uint64_t* hits,
                                  size_t hits_cap, int64_t* rule_ptr) {
    if ((nevents && !events) || (nseg && (!offsets || !rule_ptr)) || (hits_cap && !hits) ||
        nseg >= (size_t)PM_BS_MAX_NSEG || nevents > PM_BS_MAX_CAP || (hits && hits == events) ||
        (flags & ~PM_FR_KEEP) || (nrows && (!sets || ((uintptr_t)sets & 7))) || (!rows && nrows < nseg) ||
        !rules_well_formed(term_ptr, terms, nrules))
        return -2;
    const std::vector<uint32_t> gids = term_gids(term_ptr, terms, nrules);
    const size_t W = std::max<size_t>(1, (gids.size() + 63) / 64);
    if (words != W || nrows > PM_FR_MAX_WORDS / W) return -2;
    if (nseg == 0) return 0;
    auto bit_of = [&](uint32_t g) -> uint32_t {
        const auto it = std::lower_bound(gids.begin(), gids.end(), g);
        return it != gids.end() && *it == g ? (uint32_t)(it - gids.begin()) : PM_FR_NO_BIT;
    };
    auto row_of = [&](size_t j) -> int64_t {
        const int64_t row = rows ? rows[j] : (int64_t)j;
        return row >= 0 && (uint64_t)row < nrows ? row : -1;
    };
    auto has = [&](int64_t row, uint32_t bit) { return ((sets[(size_t)row * W + (bit >> 6)] >> (bit & 63)) & 1) != 0; };
    // N of every stream: one entry per (stream, bit), at its smallest position
    std::vector<New> fresh;
    for (size_t k = 0; k < nevents; ++k) {
        const uint64_t ev = events[k];
        const int64_t j = stream_of(offsets, nseg, (int64_t)(ev >> PM_BS_GID_BITS));
        if (j < 0) continue;
        const uint32_t bit = bit_of((uint32_t)(ev & PM_BS_GID_MASK));
        const int64_t row = row_of((size_t)j);
        if (bit == PM_FR_NO_BIT || row < 0 || has(row, bit)) continue;
        fresh.push_back({(uint64_t)j, bit, ev >> PM_BS_GID_BITS});
    }
    std::sort(fresh.begin(), fresh.end());
    fresh.erase(std::unique(fresh.begin(), fresh.end(),
                            [](const New& a, const New& b) { return a.stream == b.stream && a.bit == b.bit; }),
                fresh.end());
    // the rules by the bits of their positive terms
    std::vector<std::pair<uint32_t, uint32_t>> by_bit;
    for (size_t r = 0; r < nrules; ++r)
        for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k)
            if (!(terms[k] & PM_RL_NEGATED)) by_bit.push_back({bit_of(terms[k] & GID_MASK), (uint32_t)r});
    std::sort(by_bit.begin(), by_bit.end());
    size_t total = 0, at = 0;
    std::vector<uint32_t> cand;
    std::vector<uint64_t> mine;
    for (size_t j = 0; j < nseg; ++j) {
        rule_ptr[j] = (int64_t)total;
        const size_t lo = at;
        while (at < fresh.size() && fresh[at].stream == j) ++at;
        if (at == lo) continue;
        const New *nlo = fresh.data() + lo, *nhi = fresh.data() + at;
        const int64_t row = row_of(j);  // >= 0: the stream has new terms
        cand.clear();
        for (const New* n = nlo; n < nhi; ++n) {
            auto it = std::lower_bound(by_bit.begin(), by_bit.end(), std::make_pair(n->bit, 0u));
            for (; it != by_bit.end() && it->first == n->bit; ++it) cand.push_back(it->second);
        }
        std::sort(cand.begin(), cand.end());
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
        mine.clear();
        for (const uint32_t r : cand) {
            uint64_t position = 0;
            bool fires = true;
            for (uint32_t q = term_ptr[r]; fires && q < term_ptr[r + 1]; ++q) {
                const uint32_t bit = bit_of(terms[q] & GID_MASK);
                const New* n = std::lower_bound(nlo, nhi, bit, [](const New& a, uint32_t b) { return a.bit < b; });
                const bool is_new = n != nhi && n->bit == bit;
                if (terms[q] & PM_RL_NEGATED) fires = !is_new && !has(row, bit);
                else if (is_new) position = std::max(position, n->pos);
                else fires = has(row, bit);
            }
            if (fires) mine.push_back((position << PM_BS_GID_BITS) | r);  // (a candidate has a new positive term)
        }
        std::sort(mine.begin(), mine.end());
        for (const uint64_t h : mine) {
            if (total < hits_cap) hits[total] = h;
            ++total;
        }
    }
    rule_ptr[nseg] = (int64_t)total;
    if (!(flags & PM_FR_KEEP))
        for (const New& n : fresh) sets[(size_t)row_of(n.stream) * W + (n.bit >> 6)] |= 1ull << (n.bit & 63);
    return 0;
}
