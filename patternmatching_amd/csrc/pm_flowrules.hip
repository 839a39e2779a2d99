// pm_flowrules.hip -- flow rules on the device (include/pm_hip.h, "flow
// rules"): the rules whose conjunction becomes true in this
// call's bytes, over a set per flow that the caller keeps on the device, as
// position << 24 | rule hits in per-stream ranges in CSR form; then this
// call's patterns are folded into the flows' sets.
//
// Separate launches in stream order; no kernel waits on another workgroup and
// every loop is bounded by a kernel argument:
//   fill -> hash insert -> evaluate + count -> scan (3 launches, pm_bystream.hip)
//        -> evaluate + scatter -> commit (not under PM_FLOW_RULES_KEEP)
// The insert keeps the terms that are new to their flow only.  After it the
// table is frozen and the sets are read-only until the commit: both
// evaluations read them with plain loads and so find the same hits.  The
// number of events used, min(*nevents, cap), is read on the device.
//
// Memory safety does not depend on the data: a stream index is clamped into
// [0, nseg) by the insert and tested against nseg wherever a key is read back;
// a row index is tested against nrows wherever it is read; a gid at or above
// ngid has no bit and indexes nothing; a bit is tested against 64 W; an index
// range is clamped to the index array, a rule index tested against nrules, a
// term range clamped into the terms array and to 64 terms; a probe index is
// masked by the table size; a hit is stored only below hits_cap.
#include <hip/hip_runtime.h>

#include "pm_bystream_dev.h"
#include "pm_flowrules.h"

namespace {

// The row of stream j (j < nseg), or -1 where it names none: the stream is inert.
__device__ __forceinline__ int64_t fr_row(const int64_t* __restrict__ rows, int64_t nrows, uint32_t j) {
    const int64_t row = rows ? rows[j] : (int64_t)j;
    return row >= 0 && row < nrows ? row : -1;
}

// The bit of gid g, or PM_FR_NO_BIT (also for a bit that the sets' W words do not hold).
__device__ __forceinline__ uint32_t fr_bit(const uint32_t* __restrict__ gid_bit, uint32_t ngid, uint32_t words,
                                           uint32_t g) {
    const uint32_t b = g < ngid ? gid_bit[g] : PM_FR_NO_BIT;
    return b < 64u * words ? b : PM_FR_NO_BIT;
}

__device__ __forceinline__ bool fr_carried(const uint64_t* sets, int64_t row, uint32_t words, uint32_t bit) {
    return bit != PM_FR_NO_BIT && ((sets[(uint64_t)row * words + (bit >> 6)] >> (bit & 63)) & 1ull) != 0;
}

// Pass 1: rl_insert_kernel's table over the events whose gid some term names,
// whose stream has a row and whose flow does not carry the gid yet (one plain
// load of the row's word).  Claim by 64-bit compare-and-swap on an empty slot,
// linear probing over at most max_probe = the table's slots steps, the
// position folded into the slot's minimum, with the plain look before each
// atomic.
__global__ void __launch_bounds__(BS_THREADS)
fr_insert_kernel(const uint64_t* __restrict__ events, uint64_t cap, const unsigned long long* __restrict__ nevents,
                 const int64_t* __restrict__ offs, int64_t nseg, const uint32_t* __restrict__ gid_bit, uint32_t ngid,
                 uint32_t words, const uint64_t* __restrict__ sets, int64_t nrows, const int64_t* __restrict__ rows,
                 u64* keys, u64* pos, uint64_t mask, int shift, uint64_t max_probe) {
    const uint64_t used = bs_used(nevents, cap);
    const uint64_t rounded = (used + 63) & ~63ull;  // whole waves take every turn of the loop
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < rounded; i += stride) {
        const bool valid = i < used;
        const uint64_t ev = valid ? events[i] : 0;
        const uint64_t p = ev >> PM_BS_GID_BITS;
        int64_t slo, shi;
        const uint32_t j = bs_stream_of(offs, nseg, (int64_t)p, valid, slo, shi);
        const uint32_t g = (uint32_t)(ev & PM_BS_GID_MASK);
        bool take = false;
        if (j != BS_NO_STREAM) {
            const uint32_t bit = fr_bit(gid_bit, ngid, words, g);
            const int64_t row = fr_row(rows, nrows, j);
            take = bit != PM_FR_NO_BIT && row >= 0 && !fr_carried(sets, row, words, bit);
        }
        const u64 key = ((u64)j << PM_BS_GID_BITS) | g;
        uint64_t h = bs_hash(key, shift) & mask;
        bool found = false;
        for (uint64_t probe = 0; take && probe < max_probe; ++probe) {
            u64 k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == BS_EMPTY) {
                k = atomicCAS(&keys[h], BS_EMPTY, key);
                if (k == BS_EMPTY) k = key;
            }
            if (k == key) {
                found = true;
                break;
            }
            h = (h + 1) & mask;
        }
        if (found && __hip_atomic_load(&pos[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > p) atomicMin(&pos[h], (u64)p);
    }
}

// The frozen table: is (stream << 24 | gid) in it, and at which position
// (pm_rules.hip's rl_probe, which lives in that file's anonymous namespace).
__device__ __forceinline__ bool fr_probe(const u64* __restrict__ keys, const u64* __restrict__ pos, u64 key,
                                         uint64_t mask, int shift, uint64_t max_probe, u64& p) {
    uint64_t h = bs_hash(key, shift) & mask;
    for (uint64_t probe = 0; probe < max_probe; ++probe) {
        const u64 k = keys[h];
        if (k == key) {
            p = pos[h];
            return true;
        }
        if (k == BS_EMPTY) return false;
        h = (h + 1) & mask;
    }
    return false;
}

// Passes 2 and 4, over the table's slots (a power of two >= 64: whole waves).
// A slot is a term (stream, g) that is new to its flow in this call, at its
// first position p.  The wave takes its slots that index anything one at a
// time and spreads that slot's rules -- every rule with g among its positive
// terms -- over its 64 lanes, a rule per lane in turns of 64.  A lane tests
// its rule's terms other than g and stops at the first failure:
//   a positive term u passes iff the flow carries it, or the table holds
//     (stream, u) at a position q with (q, u) < (p, g) lexicographically;
//   a negated term fails iff the flow carries it or the table holds it.
// Of a rule's new positive terms exactly one has the largest (first position,
// gid): only at its slot do all the others pass, so the rule fires at most
// once per stream, there, and p is the position of the hit.  (Positions tie:
// a pattern and its proper suffix first end at the same byte.)
// SCATTER false / true: the counting and the scatter of rl_eval_kernel.
template <bool SCATTER>
__global__ void __launch_bounds__(BS_THREADS)
fr_eval_kernel(const u64* __restrict__ keys, const u64* __restrict__ pos, uint64_t table, int shift, int64_t nseg,
               const uint32_t* __restrict__ gid_bit, const uint32_t* __restrict__ idx_ptr,
               const uint32_t* __restrict__ idx_rules, const uint32_t* __restrict__ rterm_ptr,
               const uint32_t* __restrict__ rterms, uint32_t ngid, uint32_t nrules, uint32_t nidx, uint32_t nterms,
               uint32_t words, const uint64_t* __restrict__ sets, int64_t nrows, const int64_t* __restrict__ rows,
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
        int64_t row = -1;
        if (k != BS_EMPTY && kj < (u64)nseg && g < ngid) {
            row = fr_row(rows, nrows, (uint32_t)kj);
            if (row >= 0) {
                a1 = idx_ptr[g + 1];
                a1 = a1 < nidx ? a1 : nidx;
                a0 = idx_ptr[g];
                a0 = a0 < a1 ? a0 : a1;
            }
        }
        const u64 p0 = a1 > a0 ? pos[i] : 0;
        uint64_t pending = __ballot(a1 > a0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            pending &= pending - 1;
            const uint32_t lj = (uint32_t)__shfl((int)(uint32_t)kj, leader);  // < nseg < 2^31
            const uint32_t lg = (uint32_t)__shfl((int)g, leader);
            const uint32_t lbeg = (uint32_t)__shfl((int)a0, leader), lend = (uint32_t)__shfl((int)a1, leader);
            const u64 lpos = (u64)__shfl((long long)p0, leader);
            const int64_t lrow = (int64_t)__shfl((long long)row, leader);  // in [0, nrows)
            const u64 skey = (u64)lj << PM_BS_GID_BITS;
            u64 slot_hits = 0;
            for (uint32_t base = lbeg; base < lend; base += 64) {  // lend - lbeg <= nidx
                const uint32_t idx = base + (uint32_t)lane;
                bool fires = false;
                uint32_t r = 0;
                if (idx < lend) {
                    r = idx_rules[idx];
                    if (r < nrules) {
                        uint32_t t1 = rterm_ptr[r + 1];
                        t1 = t1 < nterms ? t1 : nterms;
                        uint32_t t0 = rterm_ptr[r];
                        t0 = t0 < t1 ? t0 : t1;
                        if (t1 - t0 > PM_RL_MAX_TERMS) t1 = t0 + PM_RL_MAX_TERMS;
                        fires = true;
                        for (uint32_t q = t0; fires && q < t1; ++q) {
                            const uint32_t t = rterms[q];
                            const uint32_t u = t & (uint32_t)PM_BS_GID_MASK;
                            if (u == lg) continue;  // the slot's own term
                            const bool carried = fr_carried(sets, lrow, words, fr_bit(gid_bit, ngid, words, u));
                            u64 up = 0;
                            const bool held = !carried && fr_probe(keys, pos, skey | u, mask, shift, table, up);
                            if (t & PM_RL_NEGATED) fires = !(carried || held);
                            else fires = carried || (held && (up < lpos || (up == lpos && u < lg)));
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
                        if (slot < hits_cap) hits[slot] = (lpos << PM_BS_GID_BITS) | r;
                    }
                } else {
                    slot_hits += n;
                }
            }
            if (!SCATTER && slot_hits && lane == 0) atomicAdd(&cnt[lj], slot_hits);
        }
    }
}

// Pass 5, a launch of its own behind the scatter: every occupied slot is a
// term new to its flow, and its bit is OR-ed into the flow's row.
__global__ void __launch_bounds__(BS_THREADS)
fr_commit_kernel(const u64* __restrict__ keys, uint64_t table, int64_t nseg, const uint32_t* __restrict__ gid_bit,
                 uint32_t ngid, uint32_t words, u64* sets, int64_t nrows, const int64_t* __restrict__ rows) {
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < table; i += stride) {
        const u64 k = keys[i];
        const u64 kj = k >> PM_BS_GID_BITS;
        if (k == BS_EMPTY || kj >= (u64)nseg) continue;
        const uint32_t bit = fr_bit(gid_bit, ngid, words, (uint32_t)(k & PM_BS_GID_MASK));
        const int64_t row = fr_row(rows, nrows, (uint32_t)kj);
        if (bit == PM_FR_NO_BIT || row < 0) continue;
        atomicOr(&sets[(uint64_t)row * words + (bit >> 6)], 1ull << (bit & 63));
    }
}

}  // namespace

hipError_t pm_launch_flow_rules(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                                const int64_t* offsets, int64_t nseg, const PmFlowRulesDev& rules, uint64_t* sets,
                                int64_t nrows, const int64_t* rows, bool keep, uint64_t* hits, uint64_t hits_cap,
                                int64_t* rule_ptr, void* scratch, int num_cu, hipStream_t s) {
    const PmRulesLayout l = pm_rules_layout(cap, nseg);
    char* base = (char*)scratch;
    u64* keys = (u64*)(base + l.keys_off);
    u64* pos = (u64*)(base + l.pos_off);
    u64* cnt = (u64*)(base + l.cnt_off);
    u64* bsum = (u64*)(base + l.bsum_off);
    // keys and pos lie back to back: one fill empties both
    hipError_t e = hipMemsetAsync(keys, 0xFF, 2 * (size_t)l.table * sizeof(u64), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(cnt, 0, (size_t)nseg * sizeof(u64), s);
    if (e != hipSuccess) return e;
    int shift = 64;
    for (uint64_t t = l.table; t > 1; t >>= 1) --shift;
    fr_insert_kernel<<<pm_bs_grid(cap, num_cu), BS_THREADS, 0, s>>>(events, cap, nevents, offsets, nseg, rules.gid_bit,
                                                                     rules.ngid, rules.words, sets, nrows, rows, keys,
                                                                     pos, l.table - 1, shift, l.table);
    const int tgrid = pm_bs_grid(l.table, num_cu);
    fr_eval_kernel<false><<<tgrid, BS_THREADS, 0, s>>>(keys, pos, l.table, shift, nseg, rules.gid_bit, rules.idx_ptr,
                                                        rules.idx_rules, rules.rterm_ptr, rules.rterms, rules.ngid,
                                                        rules.nrules, rules.nidx, rules.nterms, rules.words, sets, nrows,
                                                        rows, cnt, rule_ptr, hits, hits_cap);
    pm_launch_bs_scan(cnt, nseg, bsum, rule_ptr, s);
    fr_eval_kernel<true><<<tgrid, BS_THREADS, 0, s>>>(keys, pos, l.table, shift, nseg, rules.gid_bit, rules.idx_ptr,
                                                       rules.idx_rules, rules.rterm_ptr, rules.rterms, rules.ngid,
                                                       rules.nrules, rules.nidx, rules.nterms, rules.words, sets, nrows,
                                                       rows, cnt, rule_ptr, hits, hits_cap);
    if (!keep)
        fr_commit_kernel<<<tgrid, BS_THREADS, 0, s>>>(keys, l.table, nseg, rules.gid_bit, rules.ngid, rules.words,
                                                      (u64*)sets, nrows, rows);
    return hipGetLastError();
}
