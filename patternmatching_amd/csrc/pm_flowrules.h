// pm_flowrules.h -- flow rules (include/pm_hip.h, "flow rules"): what the
// device passes (pm_flowrules.hip), the host tables and twin
// (pm_flowrules_host.cpp) and the plugin's entry points share.  The scratch
// of one call is the rules call's (pm_rules.h, pm_rules_layout).
#ifndef PM_FLOWRULES_H
#define PM_FLOWRULES_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "pm_rules.h"

constexpr uint32_t PM_FR_KEEP = 1u;                  // PM_FLOW_RULES_KEEP
constexpr uint32_t PM_FR_NO_BIT = 0xFFFFFFFFu;       // gid_bit of a gid that no term names
constexpr uint64_t PM_FR_MAX_WORDS = 1ull << 40;     // nrows x W, inclusive

// The rule tables as the device walks them.  The bit of a gid is its rank
// among the distinct gids that any term names, ascending; W = max(1, ceil(K /
// 64)) words hold a flow's set.  The index runs from EVERY positive term's gid
// to the rules that carry it, ascending inside a gid's range.  A rule's terms
// are all there (each keeps PM_RL_NEGATED; nothing else above the gid): the
// PM_RULE_FAST term, else the positive term with the longest pattern (ties to
// the smaller gid), then the other positive terms, then the negated ones.
struct PmFlowRulesImage {
    std::vector<uint32_t> gid_bit;    // npat + 1, by gid (PM_FR_NO_BIT: no term)
    std::vector<uint32_t> idx_ptr;    // npat + 2, by gid
    std::vector<uint32_t> idx_rules;  // one entry per positive term
    std::vector<uint32_t> rterm_ptr;  // nrules + 1
    std::vector<uint32_t> rterms;     // every term
    uint32_t nbits = 0;               // K
    uint32_t words = 0;               // W
    uint32_t min_len = 0;             // the shortest pattern a term names
    uint32_t max_fanout = 0;          // the longest range of the index
};

// 0, or -2 for what pm_hip_set_flow_rules rejects (img is then unspecified).
int pm_flow_rules_image(const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, const uint32_t* pattern_len,
                        size_t npat, PmFlowRulesImage& img);

// The device tables of one object.
struct PmFlowRulesDev {
    const uint32_t* gid_bit = nullptr;
    const uint32_t* idx_ptr = nullptr;
    const uint32_t* idx_rules = nullptr;
    const uint32_t* rterm_ptr = nullptr;
    const uint32_t* rterms = nullptr;
    uint32_t ngid = 0;    // npat + 1: a gid at or above it has no bit and indexes nothing
    uint32_t nrules = 0;
    uint32_t nidx = 0;    // the entries of idx_rules
    uint32_t nterms = 0;  // the entries of rterms
    uint32_t words = 0;   // W
};

#ifdef __HIPCC__
// The passes of pm_hip_flow_rules_device, enqueued on s in stream order (nseg
// >= 1, cap >= 1; every pointer and nrows checked by the caller; scratch holds
// pm_rules_layout(cap, nseg).bytes).  Nothing is allocated and the host is
// never waited for.  keep: no commit pass.
hipError_t pm_launch_flow_rules(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                                const int64_t* offsets, int64_t nseg, const PmFlowRulesDev& rules, uint64_t* sets,
                                int64_t nrows, const int64_t* rows, bool keep, uint64_t* hits, uint64_t hits_cap,
                                int64_t* rule_ptr, void* scratch, int num_cu, hipStream_t s);
#endif

#endif  // PM_FLOWRULES_H
