// pm_rules.hip -- rules over per-stream sets on the device (include/pm_hip.h,
// "rules"): which multi-pattern rules fire in each stream of a
// match list, as position << 24 | rule hits in per-stream ranges in CSR form.
//
// Separate launches in stream order; no kernel waits on another workgroup and
// every loop is bounded by a kernel argument:
//   fill -> hash insert -> evaluate + count -> scan (3 launches, pm_bystream.hip)
//        -> evaluate + scatter
// After the insert the table is frozen: both evaluations read it with plain
// loads and so find the same hits.  The number of events used,
// min(*nevents, cap), is read on the device, so the call can follow a scan
// with no synchronize between.
//
// Memory safety does not depend on the data: a stream index is clamped into
// [0, nseg) by the insert and tested against nseg wherever a key is read back;
// a gid at or above ngid anchors nothing; a rule index is tested against
// nrules, a term range clamped into the terms array and to 64 terms; a probe
// index is masked by the table size; a hit is stored only below hits_cap.
#include <hip/hip_runtime.h>

#include "pm_bystream_dev.h"
#include "pm_rules.h"

namespace {

// Pass 1: bs_insert_kernel's table without the ranks and the counts.  Every
// used event that lies in a stream claims the slot of its key stream << 24 |
// gid (64-bit compare-and-swap on an empty slot; linear probing, at most
// max_probe = the table's slots steps) and folds its position into the slot's
// minimum, with the plain look before each atomic.
__global__ void __launch_bounds__(BS_THREADS)
rl_insert_kernel(const uint64_t* __restrict__ events, uint64_t cap, const unsigned long long* __restrict__ nevents,
                 const int64_t* __restrict__ offs, int64_t nseg, u64* keys, u64* pos, uint64_t mask, int shift,
                 uint64_t max_probe) {
    const uint64_t used = bs_used(nevents, cap);
    const uint64_t rounded = (used + 63) & ~63ull;  // whole waves take every turn of the loop
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < rounded; i += stride) {
        const bool valid = i < used;
        const uint64_t ev = valid ? events[i] : 0;
        const uint64_t p = ev >> PM_BS_GID_BITS;
        int64_t slo, shi;
        const uint32_t j = bs_stream_of(offs, nseg, (int64_t)p, valid, slo, shi);
        const u64 key = ((u64)j << PM_BS_GID_BITS) | (ev & PM_BS_GID_MASK);
        uint64_t h = bs_hash(key, shift) & mask;
        bool found = false;
        for (uint64_t probe = 0; j != BS_NO_STREAM && probe < max_probe; ++probe) {
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

// The frozen table: is (stream << 24 | gid) in it, and at which position.
__device__ __forceinline__ bool rl_probe(const u64* __restrict__ keys, const u64* __restrict__ pos, u64 key,
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
// Each distinct (stream, gid) sits in exactly one slot, so a rule is verified
// at most once per stream, at the slot of its anchor.  The wave takes its
// slots that anchor anything one at a time and spreads that slot's rules over
// its 64 lanes, a rule per lane in turns of 64: a gid that anchors thousands
// of rules costs its wave thousands / 64 turns, not thousands.  A lane probes
// the table for its rule's other terms, the positive ones first, stops at the
// first failure and keeps the largest first position.
// SCATTER false: the slot's hits, summed over the turns, are added to the
// stream's count by one lane (no value returned).  SCATTER true: per turn with
// hits one lane takes their number from the stream's count (counted back down,
// so it ends at 0) and the firing lanes store at their rank among the ballot
// behind rule_ptr[stream], below hits_cap only.
template <bool SCATTER>
__global__ void __launch_bounds__(BS_THREADS)
rl_eval_kernel(const u64* __restrict__ keys, const u64* __restrict__ pos, uint64_t table, int shift, int64_t nseg,
               const uint32_t* __restrict__ anchor_ptr, const uint32_t* __restrict__ anchor_rules,
               const uint32_t* __restrict__ rterm_ptr, const uint32_t* __restrict__ rterms, uint32_t ngid,
               uint32_t nrules, uint32_t nterms, u64* __restrict__ cnt, const int64_t* __restrict__ rule_ptr,
               uint64_t* __restrict__ hits, uint64_t hits_cap) {
    const uint64_t mask = table - 1;
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    const int lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < table; i += stride) {
        const u64 k = keys[i];
        const u64 kj = k >> PM_BS_GID_BITS;
        const uint32_t g = (uint32_t)(k & PM_BS_GID_MASK);
        uint32_t a0 = 0, a1 = 0;
        if (k != BS_EMPTY && kj < (u64)nseg && g < ngid) {
            a1 = anchor_ptr[g + 1];
            a1 = a1 < nrules ? a1 : nrules;
            a0 = anchor_ptr[g];
            a0 = a0 < a1 ? a0 : a1;
        }
        const u64 p0 = a1 > a0 ? pos[i] : 0;
        uint64_t pending = __ballot(a1 > a0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            pending &= pending - 1;
            const uint32_t lj = (uint32_t)__shfl((int)(uint32_t)kj, leader);  // < nseg < 2^31
            const uint32_t lbeg = (uint32_t)__shfl((int)a0, leader), lend = (uint32_t)__shfl((int)a1, leader);
            const u64 lpos = (u64)__shfl((long long)p0, leader);
            const u64 skey = (u64)lj << PM_BS_GID_BITS;
            u64 slot_hits = 0;
            for (uint32_t base = lbeg; base < lend; base += 64) {  // lend - lbeg <= nrules
                const uint32_t idx = base + (uint32_t)lane;
                bool fires = false;
                u64 hp = lpos;
                uint32_t r = 0;
                if (idx < lend) {
                    r = anchor_rules[idx];
                    if (r < nrules) {
                        uint32_t t1 = rterm_ptr[r + 1];
                        t1 = t1 < nterms ? t1 : nterms;
                        uint32_t t0 = rterm_ptr[r];
                        t0 = t0 < t1 ? t0 : t1;
                        if (t1 - t0 > PM_RL_MAX_TERMS) t1 = t0 + PM_RL_MAX_TERMS;
                        fires = true;
                        for (uint32_t q = t0; fires && q < t1; ++q) {
                            const uint32_t t = rterms[q];
                            u64 p = 0;
                            const bool held = rl_probe(keys, pos, skey | (t & PM_BS_GID_MASK), mask, shift, table, p);
                            if (t & PM_RL_NEGATED) fires = !held;
                            else if (held) hp = p > hp ? p : hp;
                            else fires = false;
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
                        if (slot < hits_cap) hits[slot] = (hp << PM_BS_GID_BITS) | r;
                    }
                } else {
                    slot_hits += n;
                }
            }
            if (!SCATTER && slot_hits && lane == 0) atomicAdd(&cnt[lj], slot_hits);
        }
    }
}

}  // namespace

hipError_t pm_launch_rules_by_stream(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                                     const int64_t* offsets, int64_t nseg, const PmRulesDev& rules, uint64_t* hits,
                                     uint64_t hits_cap, int64_t* rule_ptr, void* scratch, int num_cu, hipStream_t s) {
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
    rl_insert_kernel<<<pm_bs_grid(cap, num_cu), BS_THREADS, 0, s>>>(events, cap, nevents, offsets, nseg, keys, pos,
                                                                     l.table - 1, shift, l.table);
    const int tgrid = pm_bs_grid(l.table, num_cu);
    rl_eval_kernel<false><<<tgrid, BS_THREADS, 0, s>>>(keys, pos, l.table, shift, nseg, rules.anchor_ptr,
                                                        rules.anchor_rules, rules.rterm_ptr, rules.rterms, rules.ngid,
                                                        rules.nrules, rules.nterms, cnt, rule_ptr, hits, hits_cap);
    pm_launch_bs_scan(cnt, nseg, bsum, rule_ptr, s);
    rl_eval_kernel<true><<<tgrid, BS_THREADS, 0, s>>>(keys, pos, l.table, shift, nseg, rules.anchor_ptr,
                                                       rules.anchor_rules, rules.rterm_ptr, rules.rterms, rules.ngid,
                                                       rules.nrules, rules.nterms, cnt, rule_ptr, hits, hits_cap);
    return hipGetLastError();
}
