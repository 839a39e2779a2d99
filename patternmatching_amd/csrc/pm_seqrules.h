// pm_seqrules.h -- ordered rules (include/pm_hip.h, "ordered rules"): what the
// device passes (pm_seqrules.hip), the host tables and twin
// (pm_seqrules_host.cpp) and the plugin's entry points share.
#ifndef PM_SEQRULES_H
#define PM_SEQRULES_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "pm_bystream.h"
#include "pm_rules.h"

constexpr uint32_t PM_SQ_FREE = 0xFFFFFFFFu;     // PM_SEQ_FREE
constexpr uint32_t PM_SQ_MAX_GAP = 0x7FFFFFFFu;  // the largest distance of a link
// A range of at most this many positions is sorted by the lane that looks at
// its slot: 16 positions are 128 bytes, one cache line, and an insertion sort
// of them is at most 120 exchanges.  A longer range goes on the work list.
constexpr uint32_t PM_SQ_LANE_MAX = 16;
// The positions one workgroup sorts in LDS at a time: 4,096 x 8 bytes = 32 KiB,
// so that a CU's 160 KiB hold several workgroups.
constexpr uint32_t PM_SQ_LDS_MAX = 4096;
constexpr uint32_t PM_SQ_REC = 3;  // words of a term's record: gid | flags, gap, L

// The scratch of one call, in this order, each part rounded up to 16 bytes:
//   keys   u64 x T        the hash table's keys, stream << 24 | gid (all-ones: empty)
//   pos    u64 x T        ... the smallest position of each key
//   scnt   u64 x T        ... the used events of each key; the scatter counts it back down to 0
//   start  i64 x (T + 1)  the exclusive scan of scnt: slot h's positions are occ[start[h] .. start[h + 1])
//   occ    u64 x cap      every used event's position, grouped by slot, each range ascending after the sort
//   wl     u32 x W        the work list: the slots whose ranges are longer than PM_SQ_LANE_MAX
//   wlcur  u32 (16 bytes) its cursor, reset inside the call
//   sbsum  u64 x ceil(T / 1,024)      the block sums of the scan over the slots
//   cnt    u64 x nseg     hits per stream; the scatter counts it back down to 0
//   bsum   u64 x ceil(nseg / 1,024)   the block sums of the scan over the streams
// T = pm_bs_table_slots(cap), W = cap / (PM_SQ_LANE_MAX + 1) + 1 (the ranges are
// disjoint parts of occ, so no more of them can be that long).
struct PmSeqRulesLayout {
    uint64_t table, wl_cap;
    size_t keys_off, pos_off, scnt_off, start_off, occ_off, wl_off, wlcur_off, sbsum_off, cnt_off, bsum_off;
    size_t bytes;
};

// cap <= PM_BS_MAX_CAP, 0 <= nseg < PM_BS_MAX_NSEG (the callers check).
inline PmSeqRulesLayout pm_seq_rules_layout(uint64_t cap, int64_t nseg) {
    PmSeqRulesLayout l{};
    l.table = pm_bs_table_slots(cap);
    l.wl_cap = cap / (PM_SQ_LANE_MAX + 1) + 1;
    const size_t T = (size_t)l.table;
    size_t at = 0;
    l.keys_off = at;
    at += T * sizeof(uint64_t);
    l.pos_off = at;
    at += T * sizeof(uint64_t);
    l.scnt_off = at;
    at += T * sizeof(uint64_t);
    l.start_off = at;
    at += pm_bs_round16((T + 1) * sizeof(int64_t));
    l.occ_off = at;
    at += pm_bs_round16((size_t)cap * sizeof(uint64_t));
    l.wl_off = at;
    at += pm_bs_round16((size_t)l.wl_cap * sizeof(uint32_t));
    l.wlcur_off = at;
    at += 16;
    l.sbsum_off = at;
    at += pm_bs_round16(((T + PM_BS_SCAN_BLOCK - 1) / PM_BS_SCAN_BLOCK) * sizeof(uint64_t));
    l.cnt_off = at;
    at += pm_bs_round16((size_t)nseg * sizeof(uint64_t));
    l.bsum_off = at;
    at += pm_bs_round16((((size_t)nseg + PM_BS_SCAN_BLOCK - 1) / PM_BS_SCAN_BLOCK) * sizeof(uint64_t));
    l.bytes = at;
    return l;
}

// The rule tables as the device walks them: the inverted index of
// pm_flat_seq_rule_tables and, per rule, one record {gid | PM_RL_NEGATED, gap,
// L} per term -- every term, the anchor too -- the positive ones in listed
// order, then the negated ones, so that a walk stops at the first link that
// fails before it looks at a negation.  L is the pattern's length.
struct PmSeqRulesImage {
    std::vector<uint32_t> anchor_ptr;    // npat + 2, by gid
    std::vector<uint32_t> anchor_rules;  // nrules, grouped by anchor gid
    std::vector<uint32_t> rterm_ptr;     // nrules + 1, in records
    std::vector<uint32_t> recs;          // PM_SQ_REC words per term
    uint32_t min_len = 0;                // the shortest pattern a term names
    // The links' upper bounds (within), one word per record and in the records'
    // order, PM_SQ_FREE where a term has none; empty where no term of the set
    // has one.  They travel beside the records: the 3-word record stays.
    std::vector<uint32_t> wins;
    uint32_t within_run = 0;  // the longest run of consecutive bounded links in any rule
};

// 0, or -2 for what pm_flat_seq_rule_tables rejects (img is then unspecified).
int pm_seq_rules_image(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps, size_t nrules,
                       const uint32_t* pattern_len, size_t npat, PmSeqRulesImage& img);
// The same with withins parallel to gaps (NULL: every one PM_SQ_FREE), checked as
// pm_flat_seq_rule_tables_within checks them.
int pm_seq_rules_image_within(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                              const uint32_t* withins, size_t nrules, const uint32_t* pattern_len, size_t npat,
                              PmSeqRulesImage& img);

// The device tables of one object.
struct PmSeqRulesDev {
    const uint32_t* anchor_ptr = nullptr;
    const uint32_t* anchor_rules = nullptr;
    const uint32_t* rterm_ptr = nullptr;
    const uint32_t* recs = nullptr;
    uint32_t ngid = 0;    // npat + 1: a gid at or above it anchors nothing
    uint32_t nrules = 0;
    uint32_t nterms = 0;  // the records of recs
    const uint32_t* wins = nullptr;  // nterms words, NULL where the set has no bound
    uint32_t within_run = 0;         // > 0: the walk with an upper bound (sq_eval_within_kernel) evaluates the set
};

#ifdef __HIPCC__
// The passes of pm_hip_seq_rules_by_stream_device, enqueued on s in stream
// order (nseg >= 1, cap >= 1; every pointer checked by the caller; scratch
// holds pm_seq_rules_layout(cap, nseg).bytes).  Nothing is allocated and the
// host is never waited for.
hipError_t pm_launch_seq_rules_by_stream(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                                         const int64_t* offsets, int64_t nseg, const PmSeqRulesDev& rules,
                                         uint64_t* hits, uint64_t hits_cap, int64_t* rule_ptr, void* scratch, int num_cu,
                                         hipStream_t s);
// The index alone (the fills and passes 1 to 4, under the same conditions): on
// return the stream holds the frozen table, the slots' ranges and the sorted
// positions in scratch, and cnt is zeroed for the caller's own evaluation.
hipError_t pm_launch_seq_index(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                               const int64_t* offsets, int64_t nseg, void* scratch, int num_cu, hipStream_t s);
#endif

#endif  // PM_SEQRULES_H
