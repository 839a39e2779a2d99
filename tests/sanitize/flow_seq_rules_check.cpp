// flow_seq_rules_check.cpp -- the walk of the flow ordered rules
// (csrc/pm_flowseqwalk.h, the very functions fs_eval_kernel calls) and their
// host code (csrc/pm_flowseqrules_host.cpp) under AddressSanitizer + UBSan:
// pm_flat_flow_seq_rule_layout, pm_flow_seq_rules_image and the twin
// pm_flat_flow_seq_rules over seeded flows cut into calls, every array sized
// exactly, and the device's evaluation on the host -- every distinct (stream,
// gid) of a call walks the rules that the image's index gives for gid, elects
// the owner as the kernel does and runs pm_fsw_rule through the image's
// records, first without and then with the commit, the bits behind it --
// compared with the twin, hits and rows, call after call.  A (stream, rule)
// pair must find exactly one owner.  Prints "ok <hits>" when everything agrees.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "pm_flowseqrules.h"
#include "pm_flowseqwalk.h"
#include "pm_hip.h"

namespace {

struct Rules {
    std::vector<uint32_t> term_ptr, terms, gaps, plen;
};

Rules make_rules(std::mt19937& rng, uint32_t npat, uint32_t nrules) {
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    Rules in;
    in.plen.push_back(0);
    for (uint32_t g = 1; g <= npat; ++g) in.plen.push_back(1 + below(6));
    in.term_ptr.push_back(0);
    for (uint32_t r = 0; r < nrules; ++r) {
        const uint32_t pos = 1 + below(5), neg_gid = 1 + below(npat);
        const bool neg = below(3) == 0;
        std::vector<bool> used(npat + 1, false);
        used[neg_gid] = neg;
        uint32_t made = 0;
        for (uint32_t k = 0; k < pos; ++k) {
            bool follows = made > 0 && below(3) != 0;
            uint32_t g = 1 + below(npat);
            if (neg && g == neg_gid) g = neg_gid % npat + 1;  // npat >= 2: another gid
            if (!follows) {  // a free term needs a gid the rule has not yet
                uint32_t tries = 0;
                while (used[g] && tries++ < npat) g = g % npat + 1;
                if (used[g]) {
                    if (!made) break;
                    follows = true;
                    g = 1 + below(npat);
                    if (neg && g == neg_gid) g = neg_gid % npat + 1;
                }
            }
            used[g] = true;
            in.terms.push_back(g);
            in.gaps.push_back(follows ? below(10) : PM_SEQ_FREE);
            ++made;
            if (made == 1 && neg) {  // a negated term between a chain's head and its follower
                in.terms.push_back(neg_gid | PM_RULE_NEGATED);
                in.gaps.push_back(PM_SEQ_FREE);
            }
        }
        if (!made) {
            in.terms.push_back(neg && neg_gid == 1 ? 2u : 1u);
            in.gaps.push_back(PM_SEQ_FREE);
        }
        in.term_ptr.push_back((uint32_t)in.terms.size());
    }
    return in;
}

// One stream of one call as the walk sees it: the sorted positions of every
// gid in arrays of exactly their length, the image and the flow's row.
struct Reader {
    const PmFlowSeqRulesImage* img;
    const std::map<uint32_t, std::vector<uint64_t>>* occ_by_gid;
    std::vector<uint64_t>* row;  // S words exactly
    int64_t delta_;
    mutable const std::vector<uint64_t>* cur = nullptr;
    uint32_t term(uint32_t q) const { return img->recs.at((size_t)q * PM_SQ_REC); }
    uint32_t gap(uint32_t q) const { return img->recs.at((size_t)q * PM_SQ_REC + 1); }
    uint32_t len(uint32_t q) const { return img->recs.at((size_t)q * PM_SQ_REC + 2); }
    int64_t delta() const { return delta_; }
    // a range is (gid << 32) + index, so that occ() knows its array and checks the index
    bool range(uint32_t q, uint64_t& a, uint64_t& b) const {
        const uint32_t g = term(q) & 0xFFFFFFu;
        const auto it = occ_by_gid->find(g);
        if (it == occ_by_gid->end()) return false;
        a = (uint64_t)g << 32;
        b = a + it->second.size();
        return true;
    }
    uint64_t occ(uint64_t i) const { return occ_by_gid->at((uint32_t)(i >> 32)).at((size_t)(i & 0xFFFFFFFFu)); }
    bool carried(uint32_t q) const {
        const uint32_t bit = img->gid_bit.at(term(q) & 0xFFFFFFu);
        return bit != PM_FR_NO_BIT && ((row->at(img->nchains + (bit >> 6)) >> (bit & 63)) & 1) != 0;
    }
    uint64_t word(uint32_t c) const { return row->at(c); }
    void store(uint32_t c, uint64_t w) { row->at(c) = w; }
};

int fail(const char* what, uint32_t seed, size_t call) {
    std::printf("FAIL %s (seed %u, call %zu)\n", what, seed, call);
    return 1;
}

}  // namespace

int main() {
    size_t total_hits = 0;
    for (uint32_t seed = 0; seed < 40; ++seed) {
        std::mt19937 rng(seed);
        auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
        const uint32_t npat = 2 + below(6), nrules = 1 + below(120), nflows = 1 + below(40);
        const Rules in = make_rules(rng, npat, nrules);
        PmFlowSeqRulesImage img;
        if (pm_flow_seq_rules_image(in.term_ptr.data(), in.terms.data(), in.gaps.data(), nrules, in.plen.data(), npat,
                                    img))
            return fail("image", seed, 0);
        std::vector<uint32_t> chain_word(in.terms.size()), bit_by_gid(npat + 1);
        uint32_t C = 0, K = 0, S = 0;
        if (pm_flat_flow_seq_rule_layout(in.term_ptr.data(), in.terms.data(), in.gaps.data(), nrules, in.plen.data(),
                                         npat, chain_word.data(), bit_by_gid.data(), &C, &K, &S) ||
            C != img.nchains || K != img.nbits || S != img.words || chain_word != img.chain_word ||
            bit_by_gid != img.gid_bit)
            return fail("layout", seed, 0);
        const uint64_t big = seed % 3 == 1 ? (1ull << 32) - 20 : seed % 3 == 2 ? (1ull << 40) + 5 : 0;
        std::vector<uint64_t> had(nflows, big);               // the bytes of each flow so far
        std::vector<uint64_t> twin_rows((size_t)nflows * S, 0), walk_rows((size_t)nflows * S, 0);
        for (size_t call = 0; call < 4; ++call) {
            // the streams of this call: a shuffled part of the flows, each with a few events
            std::vector<int64_t> rows;
            for (uint32_t f = 0; f < nflows; ++f)
                if (below(4)) rows.push_back(f);
            std::shuffle(rows.begin(), rows.end(), rng);
            if (below(5) == 0) rows.push_back(-1);  // an inert stream
            const size_t nseg = rows.size();
            std::vector<int64_t> offs(nseg + 1);
            std::vector<uint64_t> pos_in(nseg), events;
            offs[0] = 1 + below(300);
            for (size_t j = 0; j < nseg; ++j) {
                const uint32_t len = below(50);
                offs[j + 1] = offs[j] + len;
                pos_in[j] = rows[j] >= 0 ? had[(size_t)rows[j]] : 7;
                for (uint32_t e = len ? below(9) : 0; e > 0; --e)
                    events.push_back(((uint64_t)(offs[j] + below(len)) << 24) | (1 + below(npat)));
            }
            std::shuffle(events.begin(), events.end(), rng);
            // the twin: a KEEP call for the count, then the commit into an array of exactly that size
            std::vector<int64_t> ptr(nseg + 1, -1), ptr2(nseg + 1, -1);
            const std::vector<uint64_t> before = twin_rows;
            if (pm_flat_flow_seq_rules(events.data(), events.size(), offs.data(), nseg, in.term_ptr.data(),
                                       in.terms.data(), in.gaps.data(), nrules, in.plen.data(), npat, twin_rows.data(),
                                       nflows, S, rows.data(), pos_in.data(), PM_FLOW_RULES_KEEP, nullptr, 0, ptr.data()))
                return fail("twin keep", seed, call);
            if (twin_rows != before) return fail("keep wrote rows", seed, call);
            std::vector<uint64_t> hits(nseg ? (size_t)ptr[nseg] : 0);
            if (pm_flat_flow_seq_rules(events.data(), events.size(), offs.data(), nseg, in.term_ptr.data(),
                                       in.terms.data(), in.gaps.data(), nrules, in.plen.data(), npat, twin_rows.data(),
                                       nflows, S, rows.data(), pos_in.data(), 0, hits.data(), hits.size(), ptr2.data()))
                return fail("twin", seed, call);
            if (ptr != ptr2) return fail("rule_ptr differs between keep and commit", seed, call);
            // the device's evaluation on the host
            std::vector<uint64_t> walk_hits;
            for (size_t j = 0; j < nseg; ++j) {
                if (rows[j] < 0) continue;
                std::map<uint32_t, std::vector<uint64_t>> occ;
                for (const uint64_t ev : events)
                    if ((int64_t)(ev >> 24) >= offs[j] && (int64_t)(ev >> 24) < offs[j + 1])
                        occ[(uint32_t)(ev & 0xFFFFFF)].push_back(ev >> 24);
                for (auto& kv : occ) {
                    std::sort(kv.second.begin(), kv.second.end());
                    kv.second.shrink_to_fit();
                }
                std::vector<uint64_t> row(walk_rows.begin() + (size_t)rows[j] * S,
                                          walk_rows.begin() + ((size_t)rows[j] + 1) * S);
                Reader t{&img, &occ, &row, (int64_t)pos_in[j] - offs[j]};
                std::vector<uint64_t> mine[2];
                std::set<uint32_t> owned;
                for (int commit = 0; commit < 2; ++commit)
                    for (const auto& kv : occ) {
                        const uint32_t g = kv.first;
                        for (uint32_t i = img.idx_ptr.at(g); i < img.idx_ptr.at(g + 1); ++i) {
                            const uint32_t r = img.idx_rules.at(i);
                            const uint32_t t0 = img.rterm_ptr.at(r), t1 = img.rterm_ptr.at(r + 1);
                            bool owner = false;
                            for (uint32_t q = t0; q < t1; ++q) {
                                const uint32_t term = t.term(q);
                                if (term & PM_RULE_NEGATED) break;
                                if ((term & 0xFFFFFFu) == g) {
                                    owner = true;
                                    break;
                                }
                                if (occ.count(term & 0xFFFFFFu)) break;
                            }
                            if (!owner) continue;
                            if (!commit && !owned.insert(r).second) return fail("two owners", seed, call);
                            uint64_t hp = 0;
                            const bool fires = commit ? pm_fsw_rule<true>(t, t0, t1, img.rule_chain.at(r),
                                                                          img.rule_chain.at(r + 1), hp)
                                                      : pm_fsw_rule<false>(t, t0, t1, img.rule_chain.at(r),
                                                                           img.rule_chain.at(r + 1), hp);
                            if (fires) mine[commit].push_back((hp << 24) | r);
                        }
                    }
                // every rule with a positive gid in the stream has an owner
                for (uint32_t r = 0; r < nrules; ++r)
                    for (uint32_t k = in.term_ptr[r]; k < in.term_ptr[r + 1]; ++k)
                        if (!(in.terms[k] & PM_RULE_NEGATED) && occ.count(in.terms[k] & 0xFFFFFFu) && !owned.count(r))
                            return fail("no owner", seed, call);
                std::sort(mine[0].begin(), mine[0].end());
                std::sort(mine[1].begin(), mine[1].end());
                if (mine[0] != mine[1]) return fail("the count pass and the commit pass differ", seed, call);
                walk_hits.insert(walk_hits.end(), mine[1].begin(), mine[1].end());
                if ((size_t)(ptr[j + 1] - ptr[j]) != mine[1].size()) return fail("a stream's count", seed, call);
                for (const auto& kv : occ) {  // the bits, behind the walk
                    const uint32_t bit = img.gid_bit.at(kv.first);
                    if (bit != PM_FR_NO_BIT) row.at(img.nchains + (bit >> 6)) |= 1ull << (bit & 63);
                }
                std::copy(row.begin(), row.end(), walk_rows.begin() + (size_t)rows[j] * S);
            }
            if (walk_hits != hits) return fail("hits", seed, call);
            if (walk_rows != twin_rows) return fail("rows", seed, call);
            total_hits += hits.size();
            for (size_t j = 0; j < nseg; ++j)
                if (rows[j] >= 0) had[(size_t)rows[j]] += (uint64_t)(offs[j + 1] - offs[j]);
        }
    }
    if (total_hits < 200) return fail("too few hits to mean anything", 0, total_hits);
    std::printf("ok %zu\n", total_hits);
    return 0;
}
