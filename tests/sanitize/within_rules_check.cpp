// within_rules_check.cpp -- the walk with an upper bound (csrc/pm_seqwalk.h,
// the very function sq_eval_within_kernel calls) and the within host code
// (csrc/pm_seqrules_host.cpp) under AddressSanitizer + UBSan:
// pm_flat_seq_rule_tables_within, pm_seq_rules_image_within and the twin
// pm_flat_seq_rules_by_stream_within over seeded inputs, every output array
// sized exactly, and the device's evaluation on the host -- every distinct
// (stream, gid) walks the rules anchored at gid through the image's records
// and bounds with pm_sw_rule, its cursors in an array of exactly the set's
// longest run -- compared with the twin, which computes feasible sets and
// shares no code with the walk.  Prints "ok <hits>" when everything agrees.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "pm_hip.h"
#include "pm_seqrules.h"
#include "pm_seqwalk.h"

namespace {

struct Input {
    std::vector<uint32_t> term_ptr, terms, gaps, withins, plen;
    std::vector<int64_t> offs;
    std::vector<uint64_t> events;
};

Input make(uint32_t seed) {
    std::mt19937 rng(seed);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    Input in;
    // few gids and short streams, so that chains are met and missed; seed 1: long chains
    const uint32_t npat = 2 + below(5), nrules = 1 + below(200), nseg = 1 + below(150);
    const uint32_t max_pos = seed == 1 ? 9 : 5;
    in.plen.push_back(0);
    for (uint32_t g = 1; g <= npat; ++g) in.plen.push_back(1 + below(6));
    in.term_ptr.push_back(0);
    for (uint32_t r = 0; r < nrules; ++r) {
        const uint32_t pos = 1 + below(max_pos), neg_gid = 1 + below(npat);
        const bool neg = below(4) == 0;
        std::vector<bool> free_used(npat + 1, false);
        free_used[neg_gid] = neg;
        const uint32_t fast = below(2) ? below(pos) : pos;
        bool have_fast = false;
        uint32_t made = 0;
        for (uint32_t k = 0; k < pos; ++k) {
            bool follows = made > 0 && below(5) != 0;
            uint32_t g = 1 + below(npat);
            if (neg && g == neg_gid) g = neg_gid % npat + 1;  // npat >= 2: another gid
            if (!follows) {  // a free term needs a gid the rule has not yet
                uint32_t tries = 0;
                while (free_used[g] && tries++ < npat) g = g % npat + 1;
                if (free_used[g]) {
                    if (!made) break;
                    follows = true;
                    g = 1 + below(npat);
                    if (neg && g == neg_gid) g = neg_gid % npat + 1;
                }
            }
            free_used[g] = true;
            const bool f = k == fast && !have_fast;
            have_fast = have_fast || f;
            in.terms.push_back(g | (f ? PM_RULE_FAST : 0u));
            const uint32_t d = below(8);
            in.gaps.push_back(follows ? d : PM_SEQ_FREE);
            in.withins.push_back(follows && below(10) < 7 ? d + in.plen[g] + below(30) : PM_SEQ_FREE);
            ++made;
            if (made == 1 && neg) {  // a negated term between a chain's head and its follower
                in.terms.push_back(neg_gid | PM_RULE_NEGATED);
                in.gaps.push_back(PM_SEQ_FREE);
                in.withins.push_back(PM_SEQ_FREE);
            }
        }
        if (!made) {
            in.terms.push_back(neg && neg_gid == 1 ? 2u : 1u);
            in.gaps.push_back(PM_SEQ_FREE);
            in.withins.push_back(PM_SEQ_FREE);
        }
        in.term_ptr.push_back((uint32_t)in.terms.size());
    }
    int64_t at = 30 + below(100);
    in.offs.push_back(at);
    for (uint32_t j = 0; j < nseg; ++j) {
        at += below(4) == 0 ? 0 : below(300);
        in.offs.push_back(at);
    }
    const uint32_t nev = below(8000);
    const uint64_t span = (uint64_t)(in.offs.back() - in.offs.front()) + 40;
    for (uint32_t k = 0; k < nev; ++k) {
        const uint64_t p = (uint64_t)in.offs.front() - 20 + rng() % span;
        in.events.push_back((p << 24) | (1 + below(npat + 1)));  // some gids name no pattern
    }
    return in;
}

// pm_seqwalk.h's accessor over host arrays: the image's records and bounds and
// one stream's sorted positions by gid, laid end to end in one array.
struct HostTables {
    const PmSeqRulesImage* img;
    const std::vector<uint32_t>* wins;  // one word per record, also where the image has none
    const std::map<uint32_t, std::pair<uint64_t, uint64_t>>* ranges;
    const std::vector<uint64_t>* positions;
    uint32_t term(uint32_t q) const { return img->recs.at((size_t)q * PM_SQ_REC); }
    uint32_t gap(uint32_t q) const { return img->recs.at((size_t)q * PM_SQ_REC + 1); }
    uint32_t len(uint32_t q) const { return img->recs.at((size_t)q * PM_SQ_REC + 2); }
    uint32_t within(uint32_t q) const { return wins->at(q); }
    bool range(uint32_t q, uint64_t& a, uint64_t& b) const {
        const auto f = ranges->find(term(q) & 0xFFFFFFu);
        if (f == ranges->end()) return false;
        a = f->second.first;
        b = f->second.second;
        return true;
    }
    uint64_t occ(uint64_t i) const { return positions->at((size_t)i); }
};

bool run(uint32_t seed, size_t& hits_seen, uint32_t& longest) {
    const Input in = make(seed);
    const size_t nrules = in.term_ptr.size() - 1, npat = in.plen.size() - 1, nseg = in.offs.size() - 1;
    std::vector<uint32_t> aptr(npat + 2), arules(nrules), aterm(nrules);
    if (pm_flat_seq_rule_tables_within(in.term_ptr.data(), in.terms.data(), in.gaps.data(), in.withins.data(), nrules,
                                       in.plen.data(), npat, aptr.data(), arules.data(), aterm.data()))
        return false;
    PmSeqRulesImage img;
    if (pm_seq_rules_image_within(in.term_ptr.data(), in.terms.data(), in.gaps.data(), in.withins.data(), nrules,
                                  in.plen.data(), npat, img))
        return false;
    if (img.anchor_ptr != aptr || img.anchor_rules != arules || img.rterm_ptr.size() != nrules + 1 ||
        img.recs.size() != (size_t)in.terms.size() * PM_SQ_REC ||
        img.wins.size() != (img.within_run ? in.terms.size() : 0))
        return false;
    longest = std::max(longest, img.within_run);
    // the twin: counted with no room, then with exact room
    std::vector<int64_t> ptr(nseg + 1), ptr2(nseg + 1);
    if (pm_flat_seq_rules_by_stream_within(in.events.data(), in.events.size(), in.offs.data(), nseg,
                                           in.term_ptr.data(), in.terms.data(), in.gaps.data(), in.withins.data(),
                                           nrules, in.plen.data(), npat, nullptr, 0, ptr.data()))
        return false;
    std::vector<uint64_t> hits((size_t)ptr[nseg]);
    if (pm_flat_seq_rules_by_stream_within(in.events.data(), in.events.size(), in.offs.data(), nseg,
                                           in.term_ptr.data(), in.terms.data(), in.gaps.data(), in.withins.data(),
                                           nrules, in.plen.data(), npat, hits.data(), hits.size(), ptr2.data()) ||
        ptr != ptr2)
        return false;
    // the device's evaluation on the host
    std::map<int64_t, std::map<uint32_t, std::vector<uint64_t>>> occ;
    for (const uint64_t ev : in.events) {
        const int64_t p = (int64_t)(ev >> 24);
        const auto it = std::upper_bound(in.offs.begin(), in.offs.end(), p);
        const int64_t j = (it - in.offs.begin()) - 1;
        if (j < 0 || j >= (int64_t)nseg) continue;
        occ[j][(uint32_t)(ev & 0xFFFFFF)].push_back((uint64_t)p);
    }
    const std::vector<uint32_t> wins = img.within_run ? img.wins : std::vector<uint32_t>(in.terms.size(), PM_SEQ_FREE);
    std::vector<uint32_t> cursors(img.within_run);  // exactly the levels the launch would give
    const uint64_t max_turns = 4 * 64 * ((uint64_t)in.events.size() + 2);
    std::vector<uint64_t> walked;
    for (size_t j = 0; j < nseg; ++j) {
        if ((int64_t)walked.size() != ptr[j]) return false;
        const auto s = occ.find((int64_t)j);
        if (s == occ.end()) continue;
        std::vector<uint64_t> positions;
        std::map<uint32_t, std::pair<uint64_t, uint64_t>> ranges;
        for (auto& kv : s->second) {
            std::sort(kv.second.begin(), kv.second.end());
            ranges[kv.first] = {positions.size(), positions.size() + kv.second.size()};
            positions.insert(positions.end(), kv.second.begin(), kv.second.end());
        }
        const HostTables t{&img, &wins, &ranges, &positions};
        std::vector<uint64_t> mine;
        for (const auto& kv : s->second) {
            const uint32_t g = kv.first;
            if (g > npat) continue;
            for (uint32_t a = aptr[g]; a < aptr[g + 1]; ++a) {
                const uint32_t r = arules[a];
                std::fill(cursors.begin(), cursors.end(), 0xDEADBEEFu);  // the walk reads no cursor it has not set
                uint64_t hp = 0;
                if (pm_sw_rule(t, img.rterm_ptr[r], img.rterm_ptr[r + 1], cursors.data(), 1u, img.within_run, max_turns,
                               hp))
                    mine.push_back((hp << 24) | r);
            }
        }
        std::sort(mine.begin(), mine.end());
        walked.insert(walked.end(), mine.begin(), mine.end());
    }
    hits_seen += hits.size();
    return walked == hits;
}

}  // namespace

int main() {
    size_t hits_seen = 0;
    uint32_t longest = 0;
    for (uint32_t seed = 1; seed <= 10; ++seed)
        if (!run(seed, hits_seen, longest)) {
            std::printf("seed %u: the walk and the twin differ\n", seed);
            return 1;
        }
    // rejected rule sets write nothing: a within on a free term; one below d + L; NULL gaps beside withins
    const uint32_t tp[2] = {0, 2}, tt[2] = {1, 2}, pl[3] = {0, 3, 3};
    const uint32_t gfree[2] = {PM_SEQ_FREE, PM_SEQ_FREE}, g0[2] = {PM_SEQ_FREE, 0};
    const uint32_t w5[2] = {PM_SEQ_FREE, 5}, w2[2] = {PM_SEQ_FREE, 2}, w3[2] = {PM_SEQ_FREE, 3};
    uint32_t ap[4] = {9, 9, 9, 9}, ar[1] = {9}, at[1] = {9};
    int64_t rp[2] = {7, 7};
    const int64_t offs[2] = {0, 10};
    const uint32_t* bad[3][2] = {{gfree, w5}, {g0, w2}, {nullptr, w5}};
    for (const auto& b : bad) {
        if (pm_flat_seq_rule_tables_within(tp, tt, b[0], b[1], 1, pl, 2, ap, ar, at) != -2 || ap[0] != 9 || ar[0] != 9 ||
            at[0] != 9)
            return 1;
        if (pm_flat_seq_rules_by_stream_within(nullptr, 0, offs, 1, tp, tt, b[0], b[1], 1, pl, 2, nullptr, 0, rp) != -2 ||
            rp[0] != 7)
            return 1;
    }
    if (pm_flat_seq_rule_tables_within(tp, tt, g0, w3, 1, pl, 2, ap, ar, at) != 0 || ap[3] != 1 || ar[0] != 0) return 1;
    if (!hits_seen || longest < 3) return 1;
    std::printf("ok %zu\n", hits_seen);
    return 0;
}
