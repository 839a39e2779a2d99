// seq_rules_check.cpp -- the ordered rules' host code
// (csrc/pm_seqrules_host.cpp) under AddressSanitizer + UBSan:
// pm_flat_seq_rule_tables, pm_seq_rules_image and the twin
// pm_flat_seq_rules_by_stream over a few seeded inputs, every output array
// sized exactly, and the device's walk on the host -- every distinct (stream,
// gid) verifies the rules anchored at gid through the image's records, with a
// lower bound in the sorted positions of a slot -- compared with the twin.
// Prints "ok <hits>" when everything agrees.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "pm_hip.h"
#include "pm_seqrules.h"

namespace {

struct Input {
    std::vector<uint32_t> term_ptr, terms, gaps, plen;
    std::vector<int64_t> offs;
    std::vector<uint64_t> events;
};

Input make(uint32_t seed) {
    std::mt19937 rng(seed);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    Input in;
    const uint32_t npat = 6 + below(8), nrules = 1 + below(300), nseg = 1 + below(200);
    in.plen.push_back(0);
    for (uint32_t g = 1; g <= npat; ++g) in.plen.push_back(1 + below(9));
    in.term_ptr.push_back(0);
    for (uint32_t r = 0; r < nrules; ++r) {
        std::vector<uint32_t> gids(npat);
        for (uint32_t g = 0; g < npat; ++g) gids[g] = g + 1;
        std::shuffle(gids.begin(), gids.end(), rng);
        // (the negated gids come from the shuffle's end, the positive ones from its first four)
        const uint32_t pos = 1 + below(4), neg = below(3) == 0 ? 1 + below(2) : 0;
        const uint32_t fast = below(2) ? below(pos) : pos;
        uint32_t fresh = 0;  // the gids taken from the shuffle so far
        for (uint32_t k = 0; k < pos; ++k) {
            const bool follows = k > 0 && below(3) != 0;
            // a following term may repeat a gid the rule has already (A ... A)
            const uint32_t g = follows && below(3) == 0 ? gids[below(fresh)] : gids[fresh++];
            in.terms.push_back(g | (k == fast ? PM_RULE_FAST : 0u));
            in.gaps.push_back(follows ? below(12) : PM_SEQ_FREE);
            if (k == 0 && neg) {  // a negated term between a chain's head and its follower
                in.terms.push_back(gids[npat - 1] | PM_RULE_NEGATED);
                in.gaps.push_back(PM_SEQ_FREE);
            }
        }
        if (neg == 2) {
            in.terms.push_back(gids[npat - 2] | PM_RULE_NEGATED);
            in.gaps.push_back(PM_SEQ_FREE);
        }
        in.term_ptr.push_back((uint32_t)in.terms.size());
    }
    int64_t at = 30 + below(100);
    in.offs.push_back(at);
    for (uint32_t j = 0; j < nseg; ++j) {
        at += below(4) == 0 ? 0 : below(90);
        in.offs.push_back(at);
    }
    const uint32_t nev = below(6000);
    const uint64_t span = (uint64_t)(in.offs.back() - in.offs.front()) + 40;
    for (uint32_t k = 0; k < nev; ++k) {
        const uint64_t p = (uint64_t)in.offs.front() - 20 + rng() % span;
        in.events.push_back((p << 24) | (1 + below(npat + 2)));  // some gids name no pattern
    }
    return in;
}

bool run(uint32_t seed, size_t& hits_seen) {
    const Input in = make(seed);
    const size_t nrules = in.term_ptr.size() - 1, npat = in.plen.size() - 1, nseg = in.offs.size() - 1;
    std::vector<uint32_t> aptr(npat + 2), arules(nrules), aterm(nrules);
    if (pm_flat_seq_rule_tables(in.term_ptr.data(), in.terms.data(), in.gaps.data(), nrules, in.plen.data(), npat,
                                aptr.data(), arules.data(), aterm.data()))
        return false;
    PmSeqRulesImage img;
    if (pm_seq_rules_image(in.term_ptr.data(), in.terms.data(), in.gaps.data(), nrules, in.plen.data(), npat, img))
        return false;
    if (img.anchor_ptr != aptr || img.anchor_rules != arules || img.rterm_ptr.size() != nrules + 1 ||
        img.recs.size() != (size_t)in.terms.size() * PM_SQ_REC)
        return false;
    // the twin: counted with no room, then with exact room
    std::vector<int64_t> ptr(nseg + 1), ptr2(nseg + 1);
    if (pm_flat_seq_rules_by_stream(in.events.data(), in.events.size(), in.offs.data(), nseg, in.term_ptr.data(),
                                    in.terms.data(), in.gaps.data(), nrules, in.plen.data(), npat, nullptr, 0,
                                    ptr.data()))
        return false;
    std::vector<uint64_t> hits((size_t)ptr[nseg]);
    if (pm_flat_seq_rules_by_stream(in.events.data(), in.events.size(), in.offs.data(), nseg, in.term_ptr.data(),
                                    in.terms.data(), in.gaps.data(), nrules, in.plen.data(), npat, hits.data(),
                                    hits.size(), ptr2.data()) ||
        ptr != ptr2)
        return false;
    // the device's walk on the host
    std::map<std::pair<int64_t, uint32_t>, std::vector<uint64_t>> occ;
    for (const uint64_t ev : in.events) {
        const int64_t p = (int64_t)(ev >> 24);
        const auto it = std::upper_bound(in.offs.begin(), in.offs.end(), p);
        const int64_t j = (it - in.offs.begin()) - 1;
        if (j < 0 || j >= (int64_t)nseg) continue;
        occ[std::make_pair(j, (uint32_t)(ev & 0xFFFFFF))].push_back((uint64_t)p);
    }
    for (auto& kv : occ) std::sort(kv.second.begin(), kv.second.end());
    std::vector<std::vector<uint64_t>> mine(nseg);
    for (const auto& kv : occ) {
        const int64_t j = kv.first.first;
        const uint32_t g = kv.first.second;
        if (g > npat) continue;
        for (uint32_t a = aptr[g]; a < aptr[g + 1]; ++a) {
            const uint32_t r = arules[a];
            uint64_t pos = 0, prev = 0;
            bool fires = true;
            for (uint32_t q = img.rterm_ptr[r]; fires && q < img.rterm_ptr[r + 1]; ++q) {
                const uint32_t t = img.recs[q * PM_SQ_REC], gap = img.recs[q * PM_SQ_REC + 1];
                const auto f = occ.find(std::make_pair(j, t & 0xFFFFFFu));
                if (t & PM_RULE_NEGATED) {
                    fires = f == occ.end();
                    continue;
                }
                if (f == occ.end()) {
                    fires = false;
                    continue;
                }
                auto it = f->second.begin();
                if (gap != PM_SEQ_FREE)
                    it = std::lower_bound(f->second.begin(), f->second.end(), prev + gap + img.recs[q * PM_SQ_REC + 2]);
                if (it == f->second.end()) {
                    fires = false;
                    continue;
                }
                prev = *it;
                pos = std::max(pos, prev);
            }
            if (fires) mine[(size_t)j].push_back((pos << 24) | r);
        }
    }
    std::vector<uint64_t> walked;
    for (size_t j = 0; j < nseg; ++j) {
        std::sort(mine[j].begin(), mine[j].end());
        if ((int64_t)walked.size() != ptr[j]) return false;
        walked.insert(walked.end(), mine[j].begin(), mine[j].end());
    }
    hits_seen += hits.size();
    return walked == hits;
}

}  // namespace

int main() {
    size_t hits_seen = 0;
    for (uint32_t seed = 1; seed <= 8; ++seed)
        if (!run(seed, hits_seen)) {
            std::printf("seed %u: the tables' walk and the twin differ\n", seed);
            return 1;
        }
    // rejected rule sets write nothing: a gid in two free terms; a gap on the first positive term
    const uint32_t tp[2] = {0, 2}, tt[2] = {1, 1}, pl[2] = {0, 3};
    const uint32_t free2[2] = {PM_SEQ_FREE, PM_SEQ_FREE}, first[2] = {0, 0}, good[2] = {PM_SEQ_FREE, 0};
    uint32_t ap[3] = {9, 9, 9}, ar[1] = {9}, at[1] = {9};
    int64_t rp[2] = {7, 7};
    const int64_t offs[2] = {0, 10};
    for (const uint32_t* gaps : {free2, first}) {
        if (pm_flat_seq_rule_tables(tp, tt, gaps, 1, pl, 1, ap, ar, at) != -2 || ap[0] != 9 || ar[0] != 9 || at[0] != 9)
            return 1;
        if (pm_flat_seq_rules_by_stream(nullptr, 0, offs, 1, tp, tt, gaps, 1, pl, 1, nullptr, 0, rp) != -2 || rp[0] != 7)
            return 1;
    }
    if (pm_flat_seq_rule_tables(tp, tt, good, 1, pl, 1, ap, ar, at) != 0 || ap[2] != 1 || ar[0] != 0 || at[0] != 0) return 1;
    const PmSeqRulesLayout l = pm_seq_rules_layout(1, 1);
    if (pm_hip_seq_rules_scratch_bytes(1, 1) != l.bytes || l.bytes != 24 * 64 + 8 * 66 + 16 + 16 + 16 + 16 + 16 + 16)
        return 1;
    if (!hits_seen) return 1;
    std::printf("ok %zu\n", hits_seen);
    return 0;
}
