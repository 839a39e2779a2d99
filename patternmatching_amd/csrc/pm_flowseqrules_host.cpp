// pm_flowseqrules_host.cpp -- the host side of the flow ordered rules
// (include/pm_hip.h, "flow ordered rules"): the layout of a progress row and
// the device tables of a rule set, the host twin of the device call and the
// scratch formula.  Plain C++: no handle, no device, no HIP.  The twin has an
// index of its own and does not use pm_flowseqwalk.h.
#include <algorithm>
#include <utility>
#include <vector>

#include "pm_flowseqrules.h"
#include "pm_hip.h"

extern "C" size_t pm_hip_flow_seq_rules_scratch_bytes(uint64_t cap, int64_t nseg) {
    if (cap > PM_BS_MAX_CAP || nseg < 0 || nseg >= PM_BS_MAX_NSEG) return (size_t)-1;
    return pm_seq_rules_layout(cap, nseg).bytes;
}

namespace {

constexpr uint32_t GID_MASK = (uint32_t)PM_BS_GID_MASK;

// The layout of a checked set: chain_word by term (the word of the chain of two
// or more positive terms headed there, else PM_FS_NO_WORD), the gids with a
// bit, ascending, and C.  A term follows the nearest positive term before it,
// so a chain is a free positive term and the following positive terms up to
// the next free one, negated terms in between skipped.
void layout_of(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps, size_t nrules,
               std::vector<uint32_t>& chain_word, std::vector<uint32_t>& bit_gids, uint32_t& nchains) {
    chain_word.assign(term_ptr[nrules], PM_FS_NO_WORD);
    bit_gids.clear();
    nchains = 0;
    for (size_t r = 0; r < nrules; ++r) {
        uint32_t head = UINT32_MAX, length = 0;
        auto close = [&]() {
            if (head == UINT32_MAX) return;
            if (length >= 2) chain_word[head] = nchains++;
            else bit_gids.push_back(terms[head] & GID_MASK);
        };
        for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k) {
            if (terms[k] & PM_RL_NEGATED) {
                bit_gids.push_back(terms[k] & GID_MASK);
            } else if (gaps[k] == PM_SQ_FREE) {
                close();
                head = k;
                length = 1;
            } else {
                ++length;
            }
        }
        close();
    }
    std::sort(bit_gids.begin(), bit_gids.end());
    bit_gids.erase(std::unique(bit_gids.begin(), bit_gids.end()), bit_gids.end());
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
    uint64_t stream, gid, pos;  // pos: the flow byte at which the occurrence ends
    bool operator<(const Occ& o) const {
        return stream != o.stream ? stream < o.stream : gid != o.gid ? gid < o.gid : pos < o.pos;
    }
};

std::pair<const Occ*, const Occ*> occ_of(const Occ* lo, const Occ* hi, uint64_t gid) {
    const Occ* a = std::lower_bound(lo, hi, gid, [](const Occ& k, uint64_t g) { return k.gid < g; });
    const Occ* b = std::upper_bound(a, hi, gid, [](uint64_t g, const Occ& k) { return g < k.gid; });
    return {a, b};
}

// The checks of the set that the ordered rules make (pm_seqrules_host.cpp), run through their public form.
bool set_well_formed(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps, size_t nrules,
                     const uint32_t* pattern_len, size_t npat) {
    if (!term_ptr || !terms || !gaps || !pattern_len || nrules == 0 || nrules > PM_RL_MAX_RULES ||
        npat >= ((size_t)1 << PM_BS_GID_BITS))
        return false;
    std::vector<uint32_t> aptr(npat + 2), arules(nrules), aterm(nrules);
    return pm_flat_seq_rule_tables(term_ptr, terms, gaps, nrules, pattern_len, npat, aptr.data(), arules.data(),
                                   aterm.data()) == 0;
}

}  // namespace

extern "C" int pm_flat_flow_seq_rule_layout(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                                            size_t nrules, const uint32_t* pattern_len, size_t npat,
                                            uint32_t* chain_word_out, uint32_t* bit_by_gid_out, uint32_t* nchains_out,
                                            uint32_t* nbits_out, uint32_t* words_out) {
    if (!chain_word_out || !bit_by_gid_out || !nchains_out || !nbits_out || !words_out ||
        !set_well_formed(term_ptr, terms, gaps, nrules, pattern_len, npat))
        return -2;
    std::vector<uint32_t> chain_word, bit_gids;
    uint32_t nchains = 0;
    layout_of(term_ptr, terms, gaps, nrules, chain_word, bit_gids, nchains);
    std::copy(chain_word.begin(), chain_word.end(), chain_word_out);
    std::fill(bit_by_gid_out, bit_by_gid_out + npat + 1, PM_FR_NO_BIT);
    for (size_t b = 0; b < bit_gids.size(); ++b) bit_by_gid_out[bit_gids[b]] = (uint32_t)b;
    *nchains_out = nchains;
    *nbits_out = (uint32_t)bit_gids.size();
    *words_out = std::max<uint32_t>(1, nchains + (uint32_t)((bit_gids.size() + 63) / 64));
    return 0;
}

int pm_flow_seq_rules_image(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps, size_t nrules,
                            const uint32_t* pattern_len, size_t npat, PmFlowSeqRulesImage& img) {
    PmSeqRulesImage seq;
    if (pm_seq_rules_image(term_ptr, terms, gaps, nrules, pattern_len, npat, seq)) return -2;
    img.rterm_ptr = std::move(seq.rterm_ptr);
    img.recs = std::move(seq.recs);
    img.min_len = seq.min_len;
    std::vector<uint32_t> bit_gids;
    layout_of(term_ptr, terms, gaps, nrules, img.chain_word, bit_gids, img.nchains);
    img.nbits = (uint32_t)bit_gids.size();
    img.words = std::max<uint32_t>(1, img.nchains + (img.nbits + 63) / 64);
    img.gid_bit.assign(npat + 1, PM_FR_NO_BIT);
    for (size_t b = 0; b < bit_gids.size(); ++b) img.gid_bit[bit_gids[b]] = (uint32_t)b;
    // rule r's chain words are consecutive: the first of them, and one past the last
    img.rule_chain.assign(nrules + 1, 0);
    for (size_t r = 0; r < nrules; ++r) {
        uint32_t n = 0;
        for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k) n += img.chain_word[k] != PM_FS_NO_WORD;
        img.rule_chain[r + 1] = img.rule_chain[r] + n;
    }
    // the index from every distinct positive gid of a rule, by counting; ascending rules inside a gid's range
    auto first_of = [&](size_t r, uint32_t k) {  // is term k the first positive term of its gid in rule r
        for (uint32_t q = term_ptr[r]; q < k; ++q)
            if (!(terms[q] & PM_RL_NEGATED) && ((terms[q] ^ terms[k]) & GID_MASK) == 0) return false;
        return true;
    };
    img.idx_ptr.assign(npat + 2, 0);
    for (size_t r = 0; r < nrules; ++r)
        for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k)
            if (!(terms[k] & PM_RL_NEGATED) && first_of(r, k)) ++img.idx_ptr[(terms[k] & GID_MASK) + 1];
    img.max_fanout = *std::max_element(img.idx_ptr.begin(), img.idx_ptr.end());
    for (size_t g = 0; g <= npat; ++g) img.idx_ptr[g + 1] += img.idx_ptr[g];
    img.idx_rules.assign(img.idx_ptr[npat + 1], 0);
    std::vector<uint32_t> at(img.idx_ptr.begin(), img.idx_ptr.end() - 1);
    for (size_t r = 0; r < nrules; ++r)
        for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k)
            if (!(terms[k] & PM_RL_NEGATED) && first_of(r, k)) img.idx_rules[at[terms[k] & GID_MASK]++] = (uint32_t)r;
    return 0;
}

// The prefix definition, stream by stream, over the carried rows: a chain's
// levels chosen so far are final, so the hits of the flow's prefix that lie in
// this call's bytes are those of the chains that reach their last level in
// this call.  Every position is a flow position here.  The rows are read as
// they were before the call throughout and written at the end.
extern "C" int pm_flat_flow_seq_rules(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                                      const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                                      size_t nrules, const uint32_t* pattern_len, size_t npat, uint64_t* prog,
                                      size_t nrows, size_t words, const int64_t* rows, const uint64_t* pos_in,
                                      uint32_t flags, uint64_t* hits, size_t hits_cap, int64_t* rule_ptr) {
    if ((nevents && !events) || (nseg && (!offsets || !rule_ptr || !pos_in)) || (hits_cap && !hits) ||
        nseg >= (size_t)PM_BS_MAX_NSEG || nevents > PM_BS_MAX_CAP || (hits && hits == events) ||
        (flags & ~PM_FR_KEEP) || (nrows && (!prog || ((uintptr_t)prog & 7))) || (!rows && nrows < nseg) ||
        !set_well_formed(term_ptr, terms, gaps, nrules, pattern_len, npat))
        return -2;
    std::vector<uint32_t> chain_word, bit_gids;
    uint32_t nchains = 0;
    layout_of(term_ptr, terms, gaps, nrules, chain_word, bit_gids, nchains);
    const size_t S = std::max<size_t>(1, nchains + (bit_gids.size() + 63) / 64);
    if (words != S || nrows > PM_FR_MAX_WORDS / S) return -2;
    if (nseg == 0) return 0;
    auto bit_of = [&](uint32_t g) -> uint32_t {
        const auto it = std::lower_bound(bit_gids.begin(), bit_gids.end(), g);
        return it != bit_gids.end() && *it == g ? (uint32_t)(it - bit_gids.begin()) : PM_FR_NO_BIT;
    };
    auto row_of = [&](size_t j) -> int64_t {
        const int64_t row = rows ? rows[j] : (int64_t)j;
        const int64_t len = offsets[j + 1] - offsets[j];
        if (row < 0 || (uint64_t)row >= nrows || len < 0 || pos_in[j] > PM_FS_MAX_BYTES ||
            (uint64_t)len > PM_FS_MAX_BYTES - pos_in[j])
            return -1;
        return row;
    };
    auto has = [&](int64_t row, uint32_t bit) {
        return bit != PM_FR_NO_BIT && ((prog[(size_t)row * S + nchains + (bit >> 6)] >> (bit & 63)) & 1) != 0;
    };
    // the index: every event inside a live stream, ascending by stream, gid and flow position
    std::vector<Occ> occ;
    occ.reserve(nevents);
    for (size_t k = 0; k < nevents; ++k) {
        const uint64_t ev = events[k];
        const int64_t j = stream_of(offsets, nseg, (int64_t)(ev >> PM_BS_GID_BITS));
        if (j < 0 || row_of((size_t)j) < 0) continue;
        occ.push_back({(uint64_t)j, ev & PM_BS_GID_MASK, (ev >> PM_BS_GID_BITS) - (uint64_t)offsets[j] + pos_in[j]});
    }
    std::sort(occ.begin(), occ.end());
    // the rules by the gids of their positive terms
    std::vector<std::pair<uint32_t, uint32_t>> by_gid;
    for (size_t r = 0; r < nrules; ++r)
        for (uint32_t k = term_ptr[r]; k < term_ptr[r + 1]; ++k)
            if (!(terms[k] & PM_RL_NEGATED)) by_gid.push_back({terms[k] & GID_MASK, (uint32_t)r});
    std::sort(by_gid.begin(), by_gid.end());
    by_gid.erase(std::unique(by_gid.begin(), by_gid.end()), by_gid.end());
    struct Store {
        size_t at;
        uint64_t word;
    };
    std::vector<Store> stores;
    size_t total = 0, at = 0;
    std::vector<uint32_t> cand;
    std::vector<uint64_t> mine;
    for (size_t j = 0; j < nseg; ++j) {
        rule_ptr[j] = (int64_t)total;
        const size_t lo = at;
        while (at < occ.size() && occ[at].stream == j) ++at;
        if (at == lo) continue;
        const Occ *klo = occ.data() + lo, *khi = occ.data() + at;
        const int64_t row = row_of(j);  // >= 0: the stream is in the index
        const uint64_t to_buffer = (uint64_t)offsets[j] - pos_in[j];  // modulo 2^64
        cand.clear();
        for (const Occ* k = klo; k < khi; ++k) {
            if (k > klo && k[-1].gid == k->gid) continue;
            auto it = std::lower_bound(by_gid.begin(), by_gid.end(), std::make_pair((uint32_t)k->gid, 0u));
            for (; it != by_gid.end() && it->first == k->gid; ++it) cand.push_back(it->second);
            const uint32_t bit = bit_of((uint32_t)k->gid);
            if (bit != PM_FR_NO_BIT && !has(row, bit))
                stores.push_back({(size_t)row * S + nchains + (bit >> 6), 1ull << (bit & 63)});
        }
        std::sort(cand.begin(), cand.end());
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
        mine.clear();
        for (const uint32_t r : cand) {
            bool fires = true, fresh = false;
            uint64_t position = 0;
            const uint32_t a = term_ptr[r], b = term_ptr[r + 1];
            for (uint32_t k = a; k < b; ++k) {
                const uint32_t g = terms[k] & GID_MASK;
                const auto range = occ_of(klo, khi, g);
                if (terms[k] & PM_RL_NEGATED) {
                    if (has(row, bit_of(g)) || range.first != range.second) fires = false;
                    continue;
                }
                if (gaps[k] != PM_SQ_FREE) continue;  // a follower: taken with its head
                if (chain_word[k] == PM_FS_NO_WORD) {  // a chain of one term
                    if (has(row, bit_of(g))) continue;
                    if (range.first == range.second) {
                        fires = false;
                    } else {
                        fresh = true;
                        position = std::max(position, range.first->pos);
                    }
                    continue;
                }
                // the chain's followers, in order: the positive terms behind the head up to the next free one
                std::vector<uint32_t> level;
                for (uint32_t q = k + 1; q < b; ++q) {
                    if (terms[q] & PM_RL_NEGATED) continue;
                    if (gaps[q] == PM_SQ_FREE) break;
                    level.push_back(q);
                }
                const size_t w = (size_t)row * S + chain_word[k];
                const uint64_t old = prog[w];
                uint64_t depth = old & 63, end = (old >> 6) - 1;
                bool started = old != 0, now = false;
                if (!started && range.first != range.second) {
                    started = true;
                    depth = 0;
                    end = range.first->pos;
                }
                while (started && depth < level.size()) {
                    const uint32_t q = level[depth], fg = terms[q] & GID_MASK;
                    const auto fr = occ_of(klo, khi, fg);
                    const uint64_t need = end + gaps[q] + pattern_len[fg];
                    const Occ* o = std::lower_bound(fr.first, fr.second, need,
                                                    [](const Occ& k2, uint64_t p) { return k2.pos < p; });
                    if (o == fr.second) break;
                    end = o->pos;
                    ++depth;
                    now = depth == level.size();
                }
                if (!started || depth < level.size()) fires = false;
                if (now) {
                    fresh = true;
                    position = std::max(position, end);
                }
                const uint64_t word = started ? ((end + 1) << 6) | depth : 0;
                if (word != old) stores.push_back({w, word});
            }
            if (fires && fresh) mine.push_back(((position + to_buffer) << PM_BS_GID_BITS) | r);
        }
        std::sort(mine.begin(), mine.end());
        for (const uint64_t h : mine) {
            if (total < hits_cap) hits[total] = h;
            ++total;
        }
    }
    rule_ptr[nseg] = (int64_t)total;
    if (!(flags & PM_FR_KEEP))
        for (const Store& s : stores) {
            if (s.at % S < nchains) prog[s.at] = s.word;
            else prog[s.at] |= s.word;
        }
    return 0;
}
