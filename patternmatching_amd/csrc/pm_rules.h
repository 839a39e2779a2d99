// pm_rules.h -- rules over per-stream sets (include/pm_hip.h, "rules"): what
// the device passes (pm_rules.hip), the host tables and twin
// (pm_rules_host.cpp) and the plugin's entry points share.
#ifndef PM_RULES_H
#define PM_RULES_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "pm_bystream.h"

constexpr uint32_t PM_RL_MAX_TERMS = 64;
constexpr size_t PM_RL_MAX_RULES = (size_t)1 << 24;
constexpr uint32_t PM_RL_NEGATED = 1u << 31;  // PM_RULE_NEGATED
constexpr uint32_t PM_RL_FAST = 1u << 30;     // PM_RULE_FAST

// The scratch of one call, in this order:
//   keys  u64 x T      the hash table's keys, stream << 24 | gid (all-ones: empty)
//   pos   u64 x T      ... the smallest position of each key
//   cnt   u64 x nseg   hits per stream; the scatter counts it back down to 0   (rounded up to 16 bytes)
//   bsum  u64 x ceil(nseg / 1,024)   the scan's block sums                     (rounded up to 16 bytes)
// T = pm_bs_table_slots(cap).
struct PmRulesLayout {
    uint64_t table;
    size_t keys_off, pos_off, cnt_off, bsum_off;
    size_t bytes;
};

// cap <= PM_BS_MAX_CAP, 0 <= nseg < PM_BS_MAX_NSEG (the callers check).
inline PmRulesLayout pm_rules_layout(uint64_t cap, int64_t nseg) {
    PmRulesLayout l{};
    l.table = pm_bs_table_slots(cap);
    l.keys_off = 0;
    l.pos_off = (size_t)l.table * sizeof(uint64_t);
    l.cnt_off = 2 * (size_t)l.table * sizeof(uint64_t);
    l.bsum_off = l.cnt_off + pm_bs_round16((size_t)nseg * sizeof(uint64_t));
    const size_t nblk = ((size_t)nseg + PM_BS_SCAN_BLOCK - 1) / PM_BS_SCAN_BLOCK;
    l.bytes = l.bsum_off + pm_bs_round16(nblk * sizeof(uint64_t));
    return l;
}

// The rule tables as the device walks them, made from pm_flat_rule_tables'
// index: a rule's terms other than its anchor, the positive ones first (each
// keeps PM_RL_NEGATED; nothing else above the gid), so that a walk stops at
// the first positive term that is missing before it looks at a negation.
struct PmRulesImage {
    std::vector<uint32_t> anchor_ptr;    // npat + 2, by gid
    std::vector<uint32_t> anchor_rules;  // nrules, grouped by anchor gid
    std::vector<uint32_t> rterm_ptr;     // nrules + 1
    std::vector<uint32_t> rterms;        // the terms other than the anchors (at least one slot)
    uint32_t min_len = 0;                // the shortest pattern a term names
};

// 0, or -2 for what pm_flat_rule_tables rejects (img is then unspecified).
int pm_rules_image(const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, const uint32_t* pattern_len,
                   size_t npat, PmRulesImage& img);

// The device tables of one object.
struct PmRulesDev {
    const uint32_t* anchor_ptr = nullptr;
    const uint32_t* anchor_rules = nullptr;
    const uint32_t* rterm_ptr = nullptr;
    const uint32_t* rterms = nullptr;
    uint32_t ngid = 0;    // npat + 1: a gid at or above it anchors nothing
    uint32_t nrules = 0;
    uint32_t nterms = 0;  // the slots of rterms
};

#ifdef __HIPCC__
// The passes of pm_hip_rules_by_stream_device, enqueued on s in stream order
// (nseg >= 1, cap >= 1; every pointer checked by the caller; scratch holds
// pm_rules_layout(cap, nseg).bytes).  Nothing is allocated and the host is
// never waited for.
hipError_t pm_launch_rules_by_stream(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                                     const int64_t* offsets, int64_t nseg, const PmRulesDev& rules, uint64_t* hits,
                                     uint64_t hits_cap, int64_t* rule_ptr, void* scratch, int num_cu, hipStream_t s);
#endif

#endif  // PM_RULES_H
