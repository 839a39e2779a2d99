// pm_flowseqrules.h -- flow ordered rules (include/pm_hip.h, "flow ordered
// rules"): what the device passes (pm_flowseqrules.hip), the host tables and
// twin (pm_flowseqrules_host.cpp) and the plugin's entry points share.  The
// scratch of one call is the ordered-rules call's (pm_seqrules.h,
// pm_seq_rules_layout).
#ifndef PM_FLOWSEQRULES_H
#define PM_FLOWSEQRULES_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "pm_flowrules.h"
#include "pm_seqrules.h"

constexpr uint32_t PM_FS_NO_WORD = 0xFFFFFFFFu;        // a term that heads no chain of two or more
constexpr uint64_t PM_FS_MAX_BYTES = 1ull << 57;       // pos_in + length above it: the stream is inert
constexpr uint32_t PM_FS_LEVEL_BITS = 6;               // a chain word is (E + 1) << 6 | level

// The rule tables as the device walks them.  The records are
// PmSeqRulesImage's: per rule one {gid | PM_RL_NEGATED, gap, L} per term, the
// positive ones in listed order, then the negated ones, so that a chain is a
// run of records: a free one, then its followers.  The chains of two or more
// positive terms are numbered by rule and then by the head's place in the
// rule; rule r's first chain has word rule_chain[r], its next one the next
// word.  The bit of a gid is its rank, ascending, among the gids named by a
// chain of one term or by a negated term.  The index runs from every DISTINCT
// positive gid of a rule to the rule, ascending inside a gid's range.
struct PmFlowSeqRulesImage {
    std::vector<uint32_t> gid_bit;     // npat + 1, by gid (PM_FR_NO_BIT: none)
    std::vector<uint32_t> idx_ptr;     // npat + 2, by gid
    std::vector<uint32_t> idx_rules;   // one entry per distinct positive gid of a rule
    std::vector<uint32_t> rterm_ptr;   // nrules + 1, in records
    std::vector<uint32_t> recs;        // PM_SQ_REC words per term
    std::vector<uint32_t> rule_chain;  // nrules + 1: the chain words of rule r are [rule_chain[r], rule_chain[r + 1])
    std::vector<uint32_t> chain_word;  // by term of the caller's terms: the word of the chain headed there, or PM_FS_NO_WORD
    uint32_t nchains = 0;              // C
    uint32_t nbits = 0;                // K
    uint32_t words = 0;                // S = max(1, C + ceil(K / 64))
    uint32_t min_len = 0;              // the shortest pattern a term names
    uint32_t max_fanout = 0;           // the longest range of the index
};

// 0, or -2 for what pm_hip_set_flow_seq_rules rejects (img is then unspecified).
int pm_flow_seq_rules_image(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps, size_t nrules,
                            const uint32_t* pattern_len, size_t npat, PmFlowSeqRulesImage& img);

// The device tables of one object.
struct PmFlowSeqRulesDev {
    const uint32_t* gid_bit = nullptr;
    const uint32_t* idx_ptr = nullptr;
    const uint32_t* idx_rules = nullptr;
    const uint32_t* rterm_ptr = nullptr;
    const uint32_t* recs = nullptr;
    const uint32_t* rule_chain = nullptr;
    uint32_t ngid = 0;     // npat + 1: a gid at or above it has no bit and indexes nothing
    uint32_t nrules = 0;
    uint32_t nidx = 0;     // the entries of idx_rules
    uint32_t nterms = 0;   // the records of recs
    uint32_t nchains = 0;  // C
    uint32_t words = 0;    // S
};

#ifdef __HIPCC__
// The passes of pm_hip_flow_seq_rules_device, enqueued on s in stream order
// (nseg >= 1, cap >= 1; every pointer and nrows checked by the caller; scratch
// holds pm_seq_rules_layout(cap, nseg).bytes).  Nothing is allocated and the
// host is never waited for.  keep: no commit.
hipError_t pm_launch_flow_seq_rules(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                                    const int64_t* offsets, int64_t nseg, const PmFlowSeqRulesDev& rules,
                                    uint64_t* prog, int64_t nrows, const int64_t* rows, const uint64_t* pos_in,
                                    bool keep, uint64_t* hits, uint64_t hits_cap, int64_t* rule_ptr, void* scratch,
                                    int num_cu, hipStream_t s);
#endif

#endif  // PM_FLOWSEQRULES_H
