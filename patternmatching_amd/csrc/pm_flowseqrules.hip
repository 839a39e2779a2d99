// pm_flowseqrules.hip -- flow ordered rules on the device (include/pm_hip.h,
// "flow ordered rules"): the ordered rules that became true in
// this call's bytes, over a progress row per flow that the caller keeps on the
// device, as position << 24 | rule hits in per-stream ranges in CSR form; then
// the rows are advanced.
//
// Separate launches in stream order; no kernel waits on another workgroup and
// every loop is bounded by a kernel argument:
//   the ordered rules' index (pm_seqrules.hip, pm_launch_seq_index: fill ->
//   insert -> scan -> scatter -> the two sorts) -> evaluate + count -> scan over
//   the streams (3 launches) -> evaluate + scatter (+ the chain words) -> the
//   bits (the last two not under PM_FLOW_RULES_KEEP)
// After the index the table and the positions are frozen and the rows are
// read-only until the scatter pass: both evaluations read them with plain
// loads and so find the same hits.  A (stream, rule) pair is evaluated by one
// lane only -- at the slot of the rule's first positive gid, in stored order,
// that the table holds for the stream -- and that lane is the only reader and
// the only writer of the pair's chain words, so the scatter pass stores them
// behind its walk with plain stores.  The bits are shared among the rules:
// they are OR-ed in by a launch of their own behind it.
//
// Memory safety does not depend on the data: beyond pm_seqrules.hip's clamps (a
// stream index tested against nseg wherever a key is read back, a gid below
// ngid, a rule index below nrules, a record index below nterms and a rule's
// range of at most 64 records, a probe index masked by the table size, a
// slot's range clamped into [0, cap], a bisection inside its clamped range, a
// hit below hits_cap) a row index is tested against nrows wherever it is
// read, a chain-word index against C and S, a bit's word against S, an index
// range against the index array, and a level against the chain's last.
#include <hip/hip_runtime.h>

#include "pm_bystream_dev.h"
#include "pm_flowseqrules.h"
#include "pm_flowseqwalk.h"

namespace {

// The row of stream j (j < nseg) and what turns its buffer positions into flow
// positions, or -1 where the stream is inert: it names no row, or the flow
// would pass 2^57 bytes.
__device__ __forceinline__ int64_t fs_row(const int64_t* __restrict__ rows, int64_t nrows,
                                          const int64_t* __restrict__ offs, const uint64_t* __restrict__ pos_in,
                                          uint32_t j, int64_t& delta) {
    const int64_t row = rows ? rows[j] : (int64_t)j;
    const int64_t lo = offs[j], len = offs[j + 1] - lo;
    const uint64_t pin = pos_in[j];
    delta = (int64_t)pin - lo;
    if (row < 0 || row >= nrows || len < 0 || pin > PM_FS_MAX_BYTES || (uint64_t)len > PM_FS_MAX_BYTES - pin) return -1;
    return row;
}

// The frozen table: the slot of (stream << 24 | gid), or false (sq_probe of
// pm_seqrules.hip, which lives in that file's anonymous namespace).
__device__ __forceinline__ bool fs_probe(const u64* __restrict__ keys, u64 key, uint64_t mask, int shift,
                                         uint64_t max_probe, uint64_t& slot) {
    uint64_t h = bs_hash(key, shift) & mask;
    for (uint64_t probe = 0; probe < max_probe; ++probe) {
        const u64 k = keys[h];
        if (k == key) {
            slot = h;
            return true;
        }
        if (k == BS_EMPTY) return false;
        h = (h + 1) & mask;
    }
    return false;
}

// What pm_flowseqwalk.h's walk reads on the device: the frozen table, the
// sorted positions, the set's records and bits and the flow's row.
struct FsWalkDev {
    const u64* __restrict__ keys;
    const int64_t* __restrict__ start;
    const u64* __restrict__ occ_;
    const uint32_t* __restrict__ recs;
    const uint32_t* __restrict__ gid_bit;
    uint64_t* row;  // S words
    uint64_t table, cap;
    u64 skey;
    int64_t delta_;
    int shift;
    uint32_t nterms, ngid, nchains, words;
    __device__ __forceinline__ size_t at(uint32_t q) const { return q < nterms ? q : nterms - 1; }
    __device__ __forceinline__ uint32_t term(uint32_t q) const { return recs[at(q) * PM_SQ_REC]; }
    __device__ __forceinline__ uint32_t gap(uint32_t q) const { return recs[at(q) * PM_SQ_REC + 1]; }
    __device__ __forceinline__ uint32_t len(uint32_t q) const { return recs[at(q) * PM_SQ_REC + 2]; }
    __device__ __forceinline__ int64_t delta() const { return delta_; }
    __device__ __forceinline__ bool range(uint32_t q, uint64_t& a, uint64_t& b) const {
        uint64_t h = 0;
        if (!fs_probe(keys, skey | (term(q) & PM_BS_GID_MASK), table - 1, shift, table, h)) return false;
        const int64_t s0 = start[h], s1 = start[h + 1];  // clamped into [0, cap] and to begin <= end
        b = s1 < 0 ? 0 : (uint64_t)s1 > cap ? cap : (uint64_t)s1;
        a = s0 < 0 ? 0 : (uint64_t)s0;
        a = a < b ? a : b;
        return true;
    }
    __device__ __forceinline__ uint64_t occ(uint64_t i) const { return occ_[i]; }
    __device__ __forceinline__ bool carried(uint32_t q) const {
        const uint32_t g = term(q) & (uint32_t)PM_BS_GID_MASK;
        const uint32_t bit = g < ngid ? gid_bit[g] : PM_FR_NO_BIT;
        const uint64_t w = (uint64_t)nchains + (bit >> 6);
        return bit != PM_FR_NO_BIT && w < words && ((row[w] >> (bit & 63)) & 1ull) != 0;
    }
    __device__ __forceinline__ uint64_t word(uint32_t c) const { return c < nchains && c < words ? row[c] : 0; }
    __device__ __forceinline__ void store(uint32_t c, uint64_t w) {
        if (c < nchains && c < words) row[c] = w;
    }
};

// Passes 5 and 7, over the table's slots (a power of two >= 64: whole waves):
// fr_eval_kernel's structure (pm_flowrules.hip).  A slot is a (stream, g) that
// this call's bytes hold.  The wave takes its slots that index anything one
// at a time and spreads that slot's rules -- every rule with g among its
// positive terms -- over its 64 lanes, a rule per lane in turns of 64.  A lane
// first walks its rule's positive records up to g's: one whose gid the table
// holds for the stream makes the lane step aside, because the lane at that
// gid's slot evaluates the pair.  The owner runs pm_flowseqwalk.h's walk.
// SCATTER false / true: the counting and the scatter of rl_eval_kernel.
// COMMIT (with SCATTER only): the walk stores the chain words it advanced.
template <bool SCATTER, bool COMMIT>
__global__ void __launch_bounds__(BS_THREADS)
fs_eval_kernel(const u64* __restrict__ keys, const int64_t* __restrict__ start, const u64* __restrict__ occ,
               uint64_t table, uint64_t cap, int shift, const int64_t* __restrict__ offs, int64_t nseg,
               const uint32_t* __restrict__ gid_bit, const uint32_t* __restrict__ idx_ptr,
               const uint32_t* __restrict__ idx_rules, const uint32_t* __restrict__ rterm_ptr,
               const uint32_t* __restrict__ recs, const uint32_t* __restrict__ rule_chain, uint32_t ngid,
               uint32_t nrules, uint32_t nidx, uint32_t nterms, uint32_t nchains, uint32_t words, uint64_t* prog,
               int64_t nrows, const int64_t* __restrict__ rows, const uint64_t* __restrict__ pos_in,
               u64* __restrict__ cnt, const int64_t* __restrict__ rule_ptr, uint64_t* __restrict__ hits,
               uint64_t hits_cap) {
    const uint64_t mask = table - 1;
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    const int lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < table; i += stride) {
        const u64 k = keys[i];
        const u64 kj = k >> PM_BS_GID_BITS;
        const uint32_t g = (uint32_t)(k & PM_BS_GID_MASK);
        uint32_t a0 = 0, a1 = 0;
        int64_t row = -1, delta = 0;
        if (k != BS_EMPTY && kj < (u64)nseg && g < ngid) {
            row = fs_row(rows, nrows, offs, pos_in, (uint32_t)kj, delta);
            if (row >= 0) {
                a1 = idx_ptr[g + 1];
                a1 = a1 < nidx ? a1 : nidx;
                a0 = idx_ptr[g];
                a0 = a0 < a1 ? a0 : a1;
            }
        }
        uint64_t pending = __ballot(a1 > a0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            pending &= pending - 1;
            const uint32_t lj = (uint32_t)__shfl((int)(uint32_t)kj, leader);  // < nseg < 2^31
            const uint32_t lg = (uint32_t)__shfl((int)g, leader);
            const uint32_t lbeg = (uint32_t)__shfl((int)a0, leader), lend = (uint32_t)__shfl((int)a1, leader);
            const int64_t lrow = (int64_t)__shfl((long long)row, leader);  // in [0, nrows)
            const int64_t ldelta = (int64_t)__shfl((long long)delta, leader);
            const u64 skey = (u64)lj << PM_BS_GID_BITS;
            FsWalkDev tables{keys, start, occ, recs, gid_bit, prog + (uint64_t)lrow * words, table, cap, skey, ldelta,
                             shift, nterms, ngid, nchains, words};
            u64 slot_hits = 0;
            for (uint32_t base = lbeg; base < lend; base += 64) {  // lend - lbeg <= nidx
                const uint32_t idx = base + (uint32_t)lane;
                bool fires = false;
                uint64_t hp = 0;
                uint32_t r = 0;
                if (idx < lend) {
                    r = idx_rules[idx];
                    if (r < nrules && nterms) {
                        uint32_t t1 = rterm_ptr[r + 1];
                        t1 = t1 < nterms ? t1 : nterms;
                        uint32_t t0 = rterm_ptr[r];
                        t0 = t0 < t1 ? t0 : t1;
                        if (t1 - t0 > PM_RL_MAX_TERMS) t1 = t0 + PM_RL_MAX_TERMS;
                        // the owner: the slot of the rule's first positive gid that the table holds
                        bool mine = false;
                        for (uint32_t q = t0; q < t1; ++q) {
                            const uint32_t t = recs[(size_t)q * PM_SQ_REC];
                            if (t & PM_RL_NEGATED) break;
                            const uint32_t u = t & (uint32_t)PM_BS_GID_MASK;
                            if (u == lg) {
                                mine = true;
                                break;
                            }
                            uint64_t h = 0;
                            if (fs_probe(keys, skey | u, mask, shift, table, h)) break;
                        }
                        if (mine) {
                            uint32_t c1 = rule_chain[r + 1];
                            c1 = c1 < nchains ? c1 : nchains;
                            uint32_t c0 = rule_chain[r];
                            c0 = c0 < c1 ? c0 : c1;
                            fires = pm_fsw_rule<COMMIT>(tables, t0, t1, c0, c1, hp);
                        }
                    }
                }
                const uint64_t fired = __ballot(fires);
                if (!fired) continue;
                const u64 n = (u64)__popcll(fired);
                if (SCATTER) {
                    u64 at = 0;
                    if (lane == 0) at = atomicAdd(&cnt[lj], (u64)0 - n) - n;
                    at = (u64)__shfl((long long)at, 0);
                    if (fires) {
                        const uint64_t slot = (uint64_t)rule_ptr[lj] + at + (u64)__popcll(fired & ((1ull << lane) - 1));
                        if (slot < hits_cap) hits[slot] = ((u64)hp << PM_BS_GID_BITS) | r;
                    }
                } else {
                    slot_hits += n;
                }
            }
            if (!SCATTER && slot_hits && lane == 0) atomicAdd(&cnt[lj], slot_hits);
        }
    }
}

// Pass 8, a launch of its own behind the scatter: every occupied slot is a
// gid that the flow holds in this call, and where the gid has a bit it is
// OR-ed into the flow's row.
__global__ void __launch_bounds__(BS_THREADS)
fs_commit_kernel(const u64* __restrict__ keys, uint64_t table, const int64_t* __restrict__ offs, int64_t nseg,
                 const uint32_t* __restrict__ gid_bit, uint32_t ngid, uint32_t nchains, uint32_t words, u64* prog,
                 int64_t nrows, const int64_t* __restrict__ rows, const uint64_t* __restrict__ pos_in) {
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < table; i += stride) {
        const u64 k = keys[i];
        const u64 kj = k >> PM_BS_GID_BITS;
        const uint32_t g = (uint32_t)(k & PM_BS_GID_MASK);
        if (k == BS_EMPTY || kj >= (u64)nseg || g >= ngid) continue;
        const uint32_t bit = gid_bit[g];
        const uint64_t w = (uint64_t)nchains + (bit >> 6);
        if (bit == PM_FR_NO_BIT || w >= words) continue;
        int64_t delta = 0;
        const int64_t row = fs_row(rows, nrows, offs, pos_in, (uint32_t)kj, delta);
        if (row < 0) continue;
        atomicOr(&prog[(uint64_t)row * words + w], 1ull << (bit & 63));
    }
}

}  // namespace

hipError_t pm_launch_flow_seq_rules(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                                    const int64_t* offsets, int64_t nseg, const PmFlowSeqRulesDev& rules,
                                    uint64_t* prog, int64_t nrows, const int64_t* rows, const uint64_t* pos_in,
                                    bool keep, uint64_t* hits, uint64_t hits_cap, int64_t* rule_ptr, void* scratch,
                                    int num_cu, hipStream_t s) {
    const PmSeqRulesLayout l = pm_seq_rules_layout(cap, nseg);
    char* base = (char*)scratch;
    const u64* keys = (const u64*)(base + l.keys_off);
    const int64_t* start = (const int64_t*)(base + l.start_off);
    const u64* occ = (const u64*)(base + l.occ_off);
    u64* cnt = (u64*)(base + l.cnt_off);
    u64* bsum = (u64*)(base + l.bsum_off);
    hipError_t e = pm_launch_seq_index(events, cap, nevents, offsets, nseg, scratch, num_cu, s);
    if (e != hipSuccess) return e;
    int shift = 64;
    for (uint64_t t = l.table; t > 1; t >>= 1) --shift;
    const int tgrid = pm_bs_grid(l.table, num_cu);
    fs_eval_kernel<false, false><<<tgrid, BS_THREADS, 0, s>>>(
        keys, start, occ, l.table, cap, shift, offsets, nseg, rules.gid_bit, rules.idx_ptr, rules.idx_rules,
        rules.rterm_ptr, rules.recs, rules.rule_chain, rules.ngid, rules.nrules, rules.nidx, rules.nterms,
        rules.nchains, rules.words, prog, nrows, rows, pos_in, cnt, rule_ptr, hits, hits_cap);
    pm_launch_bs_scan(cnt, nseg, bsum, rule_ptr, s);
    if (keep) {
        fs_eval_kernel<true, false><<<tgrid, BS_THREADS, 0, s>>>(
            keys, start, occ, l.table, cap, shift, offsets, nseg, rules.gid_bit, rules.idx_ptr, rules.idx_rules,
            rules.rterm_ptr, rules.recs, rules.rule_chain, rules.ngid, rules.nrules, rules.nidx, rules.nterms,
            rules.nchains, rules.words, prog, nrows, rows, pos_in, cnt, rule_ptr, hits, hits_cap);
        return hipGetLastError();
    }
    fs_eval_kernel<true, true><<<tgrid, BS_THREADS, 0, s>>>(
        keys, start, occ, l.table, cap, shift, offsets, nseg, rules.gid_bit, rules.idx_ptr, rules.idx_rules,
        rules.rterm_ptr, rules.recs, rules.rule_chain, rules.ngid, rules.nrules, rules.nidx, rules.nterms,
        rules.nchains, rules.words, prog, nrows, rows, pos_in, cnt, rule_ptr, hits, hits_cap);
    fs_commit_kernel<<<tgrid, BS_THREADS, 0, s>>>(keys, l.table, offsets, nseg, rules.gid_bit, rules.ngid,
                                                   rules.nchains, rules.words, (u64*)prog, nrows, rows, pos_in);
    return hipGetLastError();
}
