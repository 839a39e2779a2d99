// flow_rules_check.cpp -- the flow rules' host code
// (csrc/pm_flowrules_host.cpp) under AddressSanitizer + UBSan:
// pm_flat_flow_rule_bits, pm_flow_rules_image and the twin pm_flat_flow_rules
// over seeded flows in three calls each, every array sized exactly (the sets
// nrows x W, the rows nseg, the hits the counted number), and the device's
// walk -- driven by the image's tables, with the lexicographic test that picks
// the completing term -- compared with the twin, down to the set words.
// Prints "ok <hits>" when everything agrees.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "pm_flowrules.h"
#include "pm_hip.h"

namespace {

struct Rules {
    std::vector<uint32_t> term_ptr, terms, plen;
};

Rules make_rules(std::mt19937& rng, uint32_t npat) {
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    Rules in;
    const uint32_t nrules = 1 + below(200);
    in.plen.push_back(0);
    for (uint32_t g = 1; g <= npat; ++g) in.plen.push_back(1 + below(9));
    in.term_ptr.push_back(0);
    for (uint32_t r = 0; r < nrules; ++r) {
        std::vector<uint32_t> gids(npat);
        for (uint32_t g = 0; g < npat; ++g) gids[g] = g + 1;
        std::shuffle(gids.begin(), gids.end(), rng);
        const uint32_t pos = 1 + below(std::min(4u, npat - 2)), neg = below(3) == 0 ? 1 + below(2) : 0;
        const uint32_t fast = below(2) ? below(pos) : pos;
        for (uint32_t k = 0; k < pos; ++k) in.terms.push_back(gids[k] | (k == fast ? PM_RULE_FAST : 0u));
        for (uint32_t k = 0; k < neg; ++k) in.terms.push_back(gids[pos + k] | PM_RULE_NEGATED);
        in.term_ptr.push_back((uint32_t)in.terms.size());
    }
    return in;
}

bool run(uint32_t seed, size_t& hits_seen) {
    std::mt19937 rng(seed);
    auto below = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    const uint32_t npat = seed % 3 == 0 ? 150 : 5 + below(40);  // 150: more than 64 term gids, W > 1
    const Rules in = make_rules(rng, npat);
    const size_t nrules = in.term_ptr.size() - 1;
    std::vector<uint32_t> bits(npat + 1);
    uint32_t nbits = 0;
    if (pm_flat_flow_rule_bits(in.term_ptr.data(), in.terms.data(), nrules, npat, bits.data(), &nbits)) return false;
    PmFlowRulesImage img;
    if (pm_flow_rules_image(in.term_ptr.data(), in.terms.data(), nrules, in.plen.data(), npat, img)) return false;
    if (img.gid_bit != bits || img.nbits != nbits || img.words != std::max(1u, (nbits + 63) / 64) ||
        img.rterms.size() != in.terms.size() || img.idx_ptr.size() != npat + 2)
        return false;
    const size_t W = img.words, nrows = 1 + below(60);
    std::vector<uint64_t> sets(nrows * W, 0), walked_sets(nrows * W, 0);
    for (int call = 0; call < 3; ++call) {
        const size_t nseg = 1 + below(80);
        std::vector<int64_t> offs, rows;
        int64_t at = 30 + below(100);
        offs.push_back(at);
        std::vector<uint32_t> free_rows(nrows);
        for (size_t r = 0; r < nrows; ++r) free_rows[r] = (uint32_t)r;
        std::shuffle(free_rows.begin(), free_rows.end(), rng);
        for (size_t j = 0; j < nseg; ++j) {
            at += below(4) == 0 ? 0 : below(50);
            offs.push_back(at);
            // a row of its own, or none (out of range on either side)
            rows.push_back(j < nrows && below(8) ? (int64_t)free_rows[j] : below(2) ? -1 - (int64_t)below(3) : (int64_t)nrows + below(3));
        }
        std::vector<uint64_t> events;
        const uint32_t nev = below(3000);
        const uint64_t span = (uint64_t)(offs.back() - offs.front()) + 40;
        for (uint32_t k = 0; k < nev; ++k) {
            const uint64_t p = (uint64_t)offs.front() - 20 + rng() % span;
            events.push_back((p << 24) | (1 + below(npat + 2)));  // some gids name no pattern
        }
        // the twin: counted under KEEP with no room, then committing with exact room
        std::vector<int64_t> ptr(nseg + 1), ptr2(nseg + 1);
        const std::vector<uint64_t> before = sets;
        if (pm_flat_flow_rules(events.data(), events.size(), offs.data(), nseg, in.term_ptr.data(), in.terms.data(), nrules,
                               sets.data(), nrows, W, rows.data(), PM_FLOW_RULES_KEEP, nullptr, 0, ptr.data()) ||
            sets != before)
            return false;
        std::vector<uint64_t> hits((size_t)ptr[nseg]);
        if (pm_flat_flow_rules(events.data(), events.size(), offs.data(), nseg, in.term_ptr.data(), in.terms.data(), nrules,
                               sets.data(), nrows, W, rows.data(), 0, hits.data(), hits.size(), ptr2.data()) ||
            ptr != ptr2)
            return false;
        // the device's walk on the host: the table of the terms new to their flow, then every slot verifies the
        // rules its gid indexes
        auto row_of = [&](int64_t j) { return rows[(size_t)j] >= 0 && rows[(size_t)j] < (int64_t)nrows ? rows[(size_t)j] : -1; };
        auto carried = [&](int64_t row, uint32_t g) {
            const uint32_t b = g <= npat ? img.gid_bit[g] : PM_FR_NO_BIT;
            return b != PM_FR_NO_BIT && ((walked_sets[(size_t)row * W + (b >> 6)] >> (b & 63)) & 1) != 0;
        };
        std::map<std::pair<int64_t, uint32_t>, uint64_t> table;
        for (const uint64_t ev : events) {
            const int64_t p = (int64_t)(ev >> 24);
            const int64_t j = (std::upper_bound(offs.begin(), offs.end(), p) - offs.begin()) - 1;
            const uint32_t g = (uint32_t)(ev & 0xFFFFFF);
            if (j < 0 || j >= (int64_t)nseg || g > npat || img.gid_bit[g] == PM_FR_NO_BIT || row_of(j) < 0 ||
                carried(row_of(j), g))
                continue;
            const auto key = std::make_pair(j, g);
            const auto f = table.find(key);
            if (f == table.end() || f->second > (uint64_t)p) table[key] = (uint64_t)p;
        }
        std::vector<std::vector<uint64_t>> mine(nseg);
        for (const auto& kv : table) {
            const int64_t j = kv.first.first, row = row_of(j);
            const uint32_t g = kv.first.second;
            const uint64_t p = kv.second;
            for (uint32_t a = img.idx_ptr[g]; a < img.idx_ptr[g + 1]; ++a) {
                const uint32_t r = img.idx_rules[a];
                bool fires = true;
                for (uint32_t q = img.rterm_ptr[r]; fires && q < img.rterm_ptr[r + 1]; ++q) {
                    const uint32_t t = img.rterms[q], u = t & 0xFFFFFFu;
                    if (u == g) continue;
                    const bool c = carried(row, u);
                    const auto f = table.find(std::make_pair(j, u));
                    const bool held = f != table.end();
                    if (t & PM_RULE_NEGATED) fires = !(c || held);
                    else fires = c || (held && (f->second < p || (f->second == p && u < g)));
                }
                if (fires) mine[(size_t)j].push_back((p << 24) | r);
            }
        }
        for (const auto& kv : table) {
            const uint32_t b = img.gid_bit[kv.first.second];
            walked_sets[(size_t)row_of(kv.first.first) * W + (b >> 6)] |= 1ull << (b & 63);
        }
        std::vector<uint64_t> walked;
        for (size_t j = 0; j < nseg; ++j) {
            std::sort(mine[j].begin(), mine[j].end());
            if ((int64_t)walked.size() != ptr[j]) return false;
            walked.insert(walked.end(), mine[j].begin(), mine[j].end());
        }
        if (walked != hits || walked_sets != sets) return false;
        hits_seen += hits.size();
        // NULL rows: row j for stream j, -2 where the rows do not reach
        std::vector<uint64_t> scratch_sets = sets;
        const int rc = pm_flat_flow_rules(events.data(), events.size(), offs.data(), nseg, in.term_ptr.data(),
                                          in.terms.data(), nrules, scratch_sets.data(), nrows, W, nullptr,
                                          PM_FLOW_RULES_KEEP, nullptr, 0, ptr2.data());
        if (rc != (nrows < nseg ? -2 : 0)) return false;
    }
    return true;
}

}  // namespace

int main() {
    size_t hits_seen = 0;
    for (uint32_t seed = 1; seed <= 12; ++seed)
        if (!run(seed, hits_seen)) {
            std::printf("seed %u: the tables' walk and the twin differ\n", seed);
            return 1;
        }
    // a rejected rule set (a gid twice) writes nothing
    const uint32_t tp[2] = {0, 2}, tt[2] = {1, 1};
    uint32_t out[2] = {9, 9}, k = 9;
    if (pm_flat_flow_rule_bits(tp, tt, 1, 1, out, &k) != -2 || out[0] != 9 || out[1] != 9 || k != 9) return 1;
    if (pm_hip_flow_rules_scratch_bytes(1, 1) != 16 * 64 + 16 + 16) return 1;
    if (!hits_seen) return 1;
    std::printf("ok %zu\n", hits_seen);
    return 0;
}
