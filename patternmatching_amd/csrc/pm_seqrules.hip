// pm_seqrules.hip -- ordered rules on the device (include/pm_hip.h, "ordered
// rules"): rules whose terms must follow one another at a
// distance, as position << 24 | rule hits in per-stream ranges in CSR form.
//
// Separate launches in stream order; no kernel waits on another workgroup and
// every loop is bounded by a kernel argument:
//   fill -> hash insert with counts -> scan over the slots (3 launches,
//   pm_bystream.hip) -> scatter of the positions -> sort of the short ranges,
//   work list of the long ones -> sort of the long ranges -> evaluate + count
//   -> scan over the streams (3 launches) -> evaluate + scatter
// A set with an upper bound on some link (within) is evaluated by
// sq_eval_within_kernel, pm_seqwalk.h's exact walk, in sq_eval_kernel's place;
// everything before the evaluation is shared.
// After the insert the table's keys are frozen, after the sorts the positions:
// both evaluations read them with plain loads and so find the same hits.  The
// number of events used, min(*nevents, cap), is read on the device, and so is
// the work list's length.
//
// Memory safety does not depend on the data: beyond pm_rules.hip's clamps (a
// stream index into [0, nseg), a gid below ngid, a rule index below nrules, a
// term range inside the records and of at most 64, a probe index masked by
// the table size, a hit below hits_cap) a range read from start[] is clamped
// into [0, cap] and to begin <= end, a position is stored below cap only, a
// work-list entry is tested against the table size, and a bisection never
// leaves its clamped range.
#include <hip/hip_runtime.h>

#include "pm_bystream_dev.h"
#include "pm_seqrules.h"
#include "pm_seqwalk.h"

namespace {

// Pass 1: rl_insert_kernel's table (pm_rules.hip) with a count per slot.  Every
// used event that lies in a stream claims the slot of its key stream << 24 |
// gid (64-bit compare-and-swap on an empty slot; linear probing, at most
// max_probe = the table's slots steps), folds its position into the slot's
// minimum and adds one to the slot's count.
__global__ void __launch_bounds__(BS_THREADS)
sq_insert_kernel(const uint64_t* __restrict__ events, uint64_t cap, const unsigned long long* __restrict__ nevents,
                 const int64_t* __restrict__ offs, int64_t nseg, u64* keys, u64* pos, u64* scnt, uint64_t mask,
                 int shift, uint64_t max_probe) {
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
        if (found) {
            if (__hip_atomic_load(&pos[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > p) atomicMin(&pos[h], (u64)p);
            atomicAdd(&scnt[h], (u64)1);
        }
    }
}

// The frozen table: the slot of (stream << 24 | gid), or false (rl_probe of
// pm_rules.hip, giving the slot and not the position).
__device__ __forceinline__ bool sq_probe(const u64* __restrict__ keys, u64 key, uint64_t mask, int shift,
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

// Slot h's range of occ, clamped into [0, cap] and to begin <= end.
__device__ __forceinline__ void sq_range(const int64_t* __restrict__ start, uint64_t h, uint64_t cap, uint64_t& a,
                                         uint64_t& b) {
    const int64_t s0 = start[h], s1 = start[h + 1];
    b = s1 < 0 ? 0 : (uint64_t)s1 > cap ? cap : (uint64_t)s1;
    a = s0 < 0 ? 0 : (uint64_t)s0;
    a = a < b ? a : b;
}

// Pass 3: every used event finds its slot again in the frozen table and takes
// a rank from the slot's count (counted back down, so it ends at 0): its
// position goes to occ[start[slot] + rank], below cap only.
__global__ void __launch_bounds__(BS_THREADS)
sq_scatter_kernel(const uint64_t* __restrict__ events, uint64_t cap, const unsigned long long* __restrict__ nevents,
                  const int64_t* __restrict__ offs, int64_t nseg, const u64* __restrict__ keys, u64* scnt,
                  const int64_t* __restrict__ start, u64* __restrict__ occ, uint64_t mask, int shift,
                  uint64_t max_probe) {
    const uint64_t used = bs_used(nevents, cap);
    const uint64_t rounded = (used + 63) & ~63ull;
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < rounded; i += stride) {
        const bool valid = i < used;
        const uint64_t ev = valid ? events[i] : 0;
        const uint64_t p = ev >> PM_BS_GID_BITS;
        int64_t slo, shi;
        const uint32_t j = bs_stream_of(offs, nseg, (int64_t)p, valid, slo, shi);
        if (j == BS_NO_STREAM) continue;
        uint64_t h = 0;
        if (!sq_probe(keys, ((u64)j << PM_BS_GID_BITS) | (ev & PM_BS_GID_MASK), mask, shift, max_probe, h)) continue;
        const u64 rank = atomicAdd(&scnt[h], ~(u64)0) - 1;
        const int64_t s0 = start[h];
        const uint64_t at = (uint64_t)s0 + rank;
        if (s0 >= 0 && at < cap) occ[at] = p;
    }
}

// Pass 4a, over the table's slots (whole waves).  A range of at most
// PM_SQ_LANE_MAX positions is sorted in place by its slot's lane (insertion
// sort; almost every range has one position and costs the look alone).  The
// slots of longer ranges go on the work list: one reservation per wave -- the
// ballot of the lanes that have one, lane 0's atomic, the lanes' ranks among
// the ballot -- and a store below wl_cap only.
__global__ void __launch_bounds__(BS_THREADS)
sq_sort_short_kernel(const u64* __restrict__ keys, const int64_t* __restrict__ start, u64* __restrict__ occ,
                     uint64_t table, uint64_t cap, uint32_t* __restrict__ wl, uint32_t* wlcur, uint64_t wl_cap) {
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    const int lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < table; i += stride) {
        uint64_t a = 0, b = 0;
        if (keys[i] != BS_EMPTY) sq_range(start, i, cap, a, b);
        const uint64_t len = b - a;
        if (len > 1 && len <= PM_SQ_LANE_MAX) {
            for (uint32_t x = 1; x < (uint32_t)len; ++x) {
                const u64 v = occ[a + x];
                uint32_t y = x;
                while (y > 0 && occ[a + y - 1] > v) {
                    occ[a + y] = occ[a + y - 1];
                    --y;
                }
                occ[a + y] = v;
            }
        }
        const bool longer = len > PM_SQ_LANE_MAX;
        const uint64_t want = __ballot(longer);
        if (!want) continue;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(wlcur, (uint32_t)__popcll(want));
        base = __builtin_amdgcn_readfirstlane(base);
        if (longer) {
            const uint64_t at = (uint64_t)base + __builtin_amdgcn_mbcnt_hi((uint32_t)(want >> 32),
                                                                           __builtin_amdgcn_mbcnt_lo((uint32_t)want, 0u));
            if (at < wl_cap) wl[at] = (uint32_t)i;
        }
    }
}

// One step of the sorting network over a[0, n): the workgroup's threads take
// the pairs (i, j), i < j, of the step -- FLIP: i and its mirror image inside
// the block of k positions; otherwise i and i + k/2 -- and exchange a pair that
// is out of order.  Every exchange sorts ascending, so the positions at and
// past n, which stand for +infinity, never move: a pair with j >= n is
// skipped, and n need not be a power of two.  i grows with the pair's number,
// so a thread stops at its first i >= n.
template <bool FLIP, typename Ptr>
__device__ __forceinline__ void sq_step(Ptr a, uint64_t n, uint64_t k) {
    const uint64_t half = k >> 1;
    for (uint64_t t = threadIdx.x;; t += BS_THREADS) {  // at most n turns: i >= t
        const uint64_t in = t & (half - 1);
        const uint64_t i = ((t - in) << 1) + in;
        if (i >= n) break;
        const uint64_t j = FLIP ? (i - in) + (k - 1 - in) : i + half;
        if (j < n) {
            const u64 x = a[i], y = a[j];
            if (x > y) {
                a[i] = y;
                a[j] = x;
            }
        }
    }
}

// The steps of the network inside blocks of at most `top` positions, for a
// part a[0, n) held in LDS: the whole network up to blocks of top (FULL), or
// only the half-cleaners from blocks of top downwards, which finish a merge
// whose wider steps ran in global memory.
template <bool FULL>
__device__ __forceinline__ void sq_lds_steps(u64* a, uint32_t n, uint32_t top) {
    if (FULL) {
        for (uint32_t k = 2; k <= top; k <<= 1) {  // log2(top) (log2(top) + 1) / 2 steps
            sq_step<true>(a, n, k);
            __syncthreads();
            for (uint32_t m = k >> 1; m >= 2; m >>= 1) {
                sq_step<false>(a, n, m);
                __syncthreads();
            }
        }
    } else {
        for (uint32_t m = top; m >= 2; m >>= 1) {
            sq_step<false>(a, n, m);
            __syncthreads();
        }
    }
}

// Pass 4b: one work-list entry per workgroup and turn; the list's length is
// read here, the loop bounded by wl_cap.  A range of at most PM_SQ_LDS_MAX
// positions is sorted in LDS.  A longer one is sorted part by part in LDS and
// then merged: per doubling of the block, the steps wider than a part run in
// global memory with a workgroup barrier between them and the rest part by
// part in LDS again -- O(m log^2 m) exchanges for m positions, log^2 (m /
// 4,096) of the passes over global memory.  n, the range and the step are the
// same for all threads of a workgroup, so every barrier is met by all.
__global__ void __launch_bounds__(BS_THREADS)
sq_sort_long_kernel(const int64_t* __restrict__ start, u64* occ, uint64_t table, uint64_t cap,
                    const uint32_t* __restrict__ wl, const uint32_t* __restrict__ wlcur, uint64_t wl_cap) {
    __shared__ u64 lds[PM_SQ_LDS_MAX];
    const uint64_t have = *wlcur;
    const uint64_t n_wl = have < wl_cap ? have : wl_cap;
    for (uint64_t e = blockIdx.x; e < wl_cap; e += gridDim.x) {
        if (e >= n_wl) break;
        const uint64_t h = wl[e];
        if (h >= table) continue;
        uint64_t a = 0, b = 0;
        sq_range(start, h, cap, a, b);
        const uint64_t len = b - a;
        u64* r = occ + a;
        for (uint64_t c = 0; c < len; c += PM_SQ_LDS_MAX) {  // every part sorted in LDS
            const uint32_t n = (uint32_t)(len - c < PM_SQ_LDS_MAX ? len - c : PM_SQ_LDS_MAX);
            uint32_t top = 2;
            while (top < n) top <<= 1;
            for (uint32_t x = threadIdx.x; x < n; x += BS_THREADS) lds[x] = r[c + x];
            __syncthreads();
            sq_lds_steps<true>(lds, n, top);
            for (uint32_t x = threadIdx.x; x < n; x += BS_THREADS) r[c + x] = lds[x];
            __syncthreads();
        }
        for (uint64_t k = 2ull * PM_SQ_LDS_MAX; (k >> 1) < len; k <<= 1) {  // merges of blocks of k / 2
            sq_step<true>(r, len, k);
            __syncthreads();
            for (uint64_t m = k >> 1; m > PM_SQ_LDS_MAX; m >>= 1) {
                sq_step<false>(r, len, m);
                __syncthreads();
            }
            for (uint64_t c = 0; c < len; c += PM_SQ_LDS_MAX) {
                const uint32_t n = (uint32_t)(len - c < PM_SQ_LDS_MAX ? len - c : PM_SQ_LDS_MAX);
                for (uint32_t x = threadIdx.x; x < n; x += BS_THREADS) lds[x] = r[c + x];
                __syncthreads();
                sq_lds_steps<false>(lds, n, PM_SQ_LDS_MAX);
                for (uint32_t x = threadIdx.x; x < n; x += BS_THREADS) r[c + x] = lds[x];
                __syncthreads();
            }
        }
    }
}

// Passes 5 and 7, over the table's slots: rl_eval_kernel's structure
// (pm_rules.hip).  The wave takes its slots that anchor anything one at a time
// and spreads that slot's rules over its 64 lanes, a rule per lane in turns
// of 64.  A lane walks all of its rule's records, the positive terms in
// listed order and then the negated ones.  A free term is a probe and the
// slot's smallest position; a following term is a probe and the first
// position in the slot's sorted range at or above prev + gap + L, prev the
// position chosen for the positive term before it (64-bit: prev < 2^40, gap <
// 2^31, L < 2^32).  The walk stops at the first failure and keeps the largest
// chosen position.  SCATTER as in rl_eval_kernel.
template <bool SCATTER>
__global__ void __launch_bounds__(BS_THREADS)
sq_eval_kernel(const u64* __restrict__ keys, const u64* __restrict__ pos, const int64_t* __restrict__ start,
               const u64* __restrict__ occ, uint64_t table, uint64_t cap, int shift, int64_t nseg,
               const uint32_t* __restrict__ anchor_ptr, const uint32_t* __restrict__ anchor_rules,
               const uint32_t* __restrict__ rterm_ptr, const uint32_t* __restrict__ recs, uint32_t ngid,
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
        uint64_t pending = __ballot(a1 > a0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            pending &= pending - 1;
            const uint32_t lj = (uint32_t)__shfl((int)(uint32_t)kj, leader);  // < nseg < 2^31
            const uint32_t lbeg = (uint32_t)__shfl((int)a0, leader), lend = (uint32_t)__shfl((int)a1, leader);
            const u64 skey = (u64)lj << PM_BS_GID_BITS;
            u64 slot_hits = 0;
            for (uint32_t base = lbeg; base < lend; base += 64) {  // lend - lbeg <= nrules
                const uint32_t idx = base + (uint32_t)lane;
                bool fires = false;
                u64 hp = 0;
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
                        u64 prev = 0;
                        for (uint32_t q = t0; fires && q < t1; ++q) {
                            const uint32_t t = recs[(size_t)q * PM_SQ_REC];
                            const uint32_t gap = recs[(size_t)q * PM_SQ_REC + 1];
                            uint64_t h = 0;
                            const bool held = sq_probe(keys, skey | (t & PM_BS_GID_MASK), mask, shift, table, h);
                            if (t & PM_RL_NEGATED) {
                                fires = !held;
                            } else if (!held) {
                                fires = false;
                            } else if (gap == PM_SQ_FREE) {
                                prev = pos[h];
                                hp = prev > hp ? prev : hp;
                            } else {
                                const u64 need = prev + (u64)gap + (u64)recs[(size_t)q * PM_SQ_REC + 2];
                                uint64_t lo, end;
                                sq_range(start, h, cap, lo, end);
                                uint64_t hi = end;
                                while (lo < hi) {  // at most log2(cap) + 1 turns
                                    const uint64_t mid = lo + ((hi - lo) >> 1);
                                    if (occ[mid] < need) lo = mid + 1;
                                    else hi = mid;
                                }
                                if (lo < end) {
                                    prev = occ[lo];
                                    hp = prev > hp ? prev : hp;
                                } else {
                                    fires = false;
                                }
                            }
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

// What pm_seqwalk.h's walk reads on the device: the frozen table, the sorted
// positions and the set's records and bounds.  A record index is clamped below
// nterms; a range is sq_range's, inside [0, cap].
struct SqWalkDev {
    const u64* __restrict__ keys;
    const int64_t* __restrict__ start;
    const u64* __restrict__ occ_;
    const uint32_t* __restrict__ recs;
    const uint32_t* __restrict__ wins;
    uint64_t table, cap;
    u64 skey;
    int shift;
    uint32_t nterms;
    __device__ __forceinline__ size_t at(uint32_t q) const { return q < nterms ? q : nterms - 1; }
    __device__ __forceinline__ uint32_t term(uint32_t q) const { return recs[at(q) * PM_SQ_REC]; }
    __device__ __forceinline__ uint32_t gap(uint32_t q) const { return recs[at(q) * PM_SQ_REC + 1]; }
    __device__ __forceinline__ uint32_t len(uint32_t q) const { return recs[at(q) * PM_SQ_REC + 2]; }
    __device__ __forceinline__ uint32_t within(uint32_t q) const { return wins[at(q)]; }
    __device__ __forceinline__ bool range(uint32_t q, uint64_t& a, uint64_t& b) const {
        uint64_t h = 0;
        if (!sq_probe(keys, skey | (term(q) & PM_BS_GID_MASK), table - 1, shift, table, h)) return false;
        sq_range(start, h, cap, a, b);
        return true;
    }
    __device__ __forceinline__ uint64_t occ(uint64_t i) const { return occ_[i]; }
};

// Passes 5 and 7 of a set with at least one bounded link: sq_eval_kernel's
// structure with pm_seqwalk.h's walk inside a rule.  The cursors of a lane's
// run lie in dynamic LDS as u32, [level][thread]: a lane's bank is its lane
// number whatever level it is on, so lanes on different levels never
// conflict.  max_run levels (BS_THREADS x 4 x max_run bytes) come with the
// launch; a run longer than that does not fire (the host sized it: none is).
// max_turns bounds the walk's loop.
template <bool SCATTER>
__global__ void __launch_bounds__(BS_THREADS)
sq_eval_within_kernel(const u64* __restrict__ keys, const int64_t* __restrict__ start, const u64* __restrict__ occ,
                      uint64_t table, uint64_t cap, int shift, int64_t nseg, const uint32_t* __restrict__ anchor_ptr,
                      const uint32_t* __restrict__ anchor_rules, const uint32_t* __restrict__ rterm_ptr,
                      const uint32_t* __restrict__ recs, const uint32_t* __restrict__ wins, uint32_t ngid,
                      uint32_t nrules, uint32_t nterms, uint32_t max_run, uint64_t max_turns, u64* __restrict__ cnt,
                      const int64_t* __restrict__ rule_ptr, uint64_t* __restrict__ hits, uint64_t hits_cap) {
    extern __shared__ uint32_t sq_cursors[];
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
        uint64_t pending = __ballot(a1 > a0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            pending &= pending - 1;
            const uint32_t lj = (uint32_t)__shfl((int)(uint32_t)kj, leader);  // < nseg < 2^31
            const uint32_t lbeg = (uint32_t)__shfl((int)a0, leader), lend = (uint32_t)__shfl((int)a1, leader);
            const SqWalkDev tables{keys, start, occ, recs, wins, table, cap, (u64)lj << PM_BS_GID_BITS, shift, nterms};
            u64 slot_hits = 0;
            for (uint32_t base = lbeg; base < lend; base += 64) {  // lend - lbeg <= nrules
                const uint32_t idx = base + (uint32_t)lane;
                bool fires = false;
                uint64_t hp = 0;
                uint32_t r = 0;
                if (idx < lend) {
                    r = anchor_rules[idx];
                    if (r < nrules && nterms) {
                        uint32_t t1 = rterm_ptr[r + 1];
                        t1 = t1 < nterms ? t1 : nterms;
                        uint32_t t0 = rterm_ptr[r];
                        t0 = t0 < t1 ? t0 : t1;
                        if (t1 - t0 > PM_RL_MAX_TERMS) t1 = t0 + PM_RL_MAX_TERMS;
                        fires = t1 > t0 &&
                                pm_sw_rule(tables, t0, t1, sq_cursors + threadIdx.x, BS_THREADS, max_run, max_turns, hp);
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

}  // namespace

// The index alone, for a caller with an evaluation of its own
// (pm_flowseqrules.hip): the fills and passes 1 to 4 of the launcher below, which
// keeps its own copy of them: the two are to be kept in step.
hipError_t pm_launch_seq_index(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                               const int64_t* offsets, int64_t nseg, void* scratch, int num_cu, hipStream_t s) {
    const PmSeqRulesLayout l = pm_seq_rules_layout(cap, nseg);
    char* base = (char*)scratch;
    u64* keys = (u64*)(base + l.keys_off);
    u64* pos = (u64*)(base + l.pos_off);
    u64* scnt = (u64*)(base + l.scnt_off);
    int64_t* start = (int64_t*)(base + l.start_off);
    u64* occ = (u64*)(base + l.occ_off);
    uint32_t* wl = (uint32_t*)(base + l.wl_off);
    uint32_t* wlcur = (uint32_t*)(base + l.wlcur_off);
    u64* sbsum = (u64*)(base + l.sbsum_off);
    u64* cnt = (u64*)(base + l.cnt_off);
    hipError_t e = hipMemsetAsync(keys, 0xFF, 2 * (size_t)l.table * sizeof(u64), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(scnt, 0, (size_t)l.table * sizeof(u64), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(wlcur, 0, 16, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(cnt, 0, (size_t)nseg * sizeof(u64), s);
    if (e != hipSuccess) return e;
    int shift = 64;
    for (uint64_t t = l.table; t > 1; t >>= 1) --shift;
    const int egrid = pm_bs_grid(cap, num_cu), tgrid = pm_bs_grid(l.table, num_cu);
    sq_insert_kernel<<<egrid, BS_THREADS, 0, s>>>(events, cap, nevents, offsets, nseg, keys, pos, scnt, l.table - 1,
                                                   shift, l.table);
    pm_launch_bs_scan(scnt, (int64_t)l.table, sbsum, start, s);
    sq_scatter_kernel<<<egrid, BS_THREADS, 0, s>>>(events, cap, nevents, offsets, nseg, keys, scnt, start, occ,
                                                    l.table - 1, shift, l.table);
    sq_sort_short_kernel<<<tgrid, BS_THREADS, 0, s>>>(keys, start, occ, l.table, cap, wl, wlcur, l.wl_cap);
    sq_sort_long_kernel<<<pm_bs_grid(l.wl_cap * BS_THREADS, num_cu), BS_THREADS, 0, s>>>(start, occ, l.table, cap, wl,
                                                                                         wlcur, l.wl_cap);
    return hipGetLastError();
}

hipError_t pm_launch_seq_rules_by_stream(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                                         const int64_t* offsets, int64_t nseg, const PmSeqRulesDev& rules,
                                         uint64_t* hits, uint64_t hits_cap, int64_t* rule_ptr, void* scratch, int num_cu,
                                         hipStream_t s) {
    const PmSeqRulesLayout l = pm_seq_rules_layout(cap, nseg);
    char* base = (char*)scratch;
    u64* keys = (u64*)(base + l.keys_off);
    u64* pos = (u64*)(base + l.pos_off);
    u64* scnt = (u64*)(base + l.scnt_off);
    int64_t* start = (int64_t*)(base + l.start_off);
    u64* occ = (u64*)(base + l.occ_off);
    uint32_t* wl = (uint32_t*)(base + l.wl_off);
    uint32_t* wlcur = (uint32_t*)(base + l.wlcur_off);
    u64* sbsum = (u64*)(base + l.sbsum_off);
    u64* cnt = (u64*)(base + l.cnt_off);
    u64* bsum = (u64*)(base + l.bsum_off);
    // the fills and passes 1 to 4 below are also pm_launch_seq_index's, above: a change to the index goes into both
    // keys and pos lie back to back: one fill empties both
    hipError_t e = hipMemsetAsync(keys, 0xFF, 2 * (size_t)l.table * sizeof(u64), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(scnt, 0, (size_t)l.table * sizeof(u64), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(wlcur, 0, 16, s);  // the work list starts empty in every call, a graph's replay too
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(cnt, 0, (size_t)nseg * sizeof(u64), s);
    if (e != hipSuccess) return e;
    int shift = 64;
    for (uint64_t t = l.table; t > 1; t >>= 1) --shift;
    const int egrid = pm_bs_grid(cap, num_cu), tgrid = pm_bs_grid(l.table, num_cu);
    sq_insert_kernel<<<egrid, BS_THREADS, 0, s>>>(events, cap, nevents, offsets, nseg, keys, pos, scnt, l.table - 1,
                                                   shift, l.table);
    pm_launch_bs_scan(scnt, (int64_t)l.table, sbsum, start, s);
    sq_scatter_kernel<<<egrid, BS_THREADS, 0, s>>>(events, cap, nevents, offsets, nseg, keys, scnt, start, occ,
                                                    l.table - 1, shift, l.table);
    sq_sort_short_kernel<<<tgrid, BS_THREADS, 0, s>>>(keys, start, occ, l.table, cap, wl, wlcur, l.wl_cap);
    // the work list is seldom long: a grid of its capacity, at most one grid of the device
    sq_sort_long_kernel<<<pm_bs_grid(l.wl_cap * BS_THREADS, num_cu), BS_THREADS, 0, s>>>(start, occ, l.table, cap, wl,
                                                                                         wlcur, l.wl_cap);
    if (rules.within_run) {
        // a set with a bound: the exact walk, one u32 cursor per level of a run and thread in LDS.  A turn of
        // the walk moves a cursor forward, touches a level for the first time or follows from such a turn: at
        // most 64 ranges of at most cap positions
        const uint32_t run = rules.within_run < PM_RL_MAX_TERMS ? rules.within_run : PM_RL_MAX_TERMS - 1;
        const size_t lds = (size_t)BS_THREADS * sizeof(uint32_t) * run;
        const uint64_t max_turns = 4 * (uint64_t)PM_RL_MAX_TERMS * (cap + 2);
        sq_eval_within_kernel<false><<<tgrid, BS_THREADS, lds, s>>>(
            keys, start, occ, l.table, cap, shift, nseg, rules.anchor_ptr, rules.anchor_rules, rules.rterm_ptr,
            rules.recs, rules.wins, rules.ngid, rules.nrules, rules.nterms, run, max_turns, cnt, rule_ptr, hits,
            hits_cap);
        pm_launch_bs_scan(cnt, nseg, bsum, rule_ptr, s);
        sq_eval_within_kernel<true><<<tgrid, BS_THREADS, lds, s>>>(
            keys, start, occ, l.table, cap, shift, nseg, rules.anchor_ptr, rules.anchor_rules, rules.rterm_ptr,
            rules.recs, rules.wins, rules.ngid, rules.nrules, rules.nterms, run, max_turns, cnt, rule_ptr, hits,
            hits_cap);
        return hipGetLastError();
    }
    sq_eval_kernel<false><<<tgrid, BS_THREADS, 0, s>>>(keys, pos, start, occ, l.table, cap, shift, nseg,
                                                        rules.anchor_ptr, rules.anchor_rules, rules.rterm_ptr,
                                                        rules.recs, rules.ngid, rules.nrules, rules.nterms, cnt,
                                                        rule_ptr, hits, hits_cap);
    pm_launch_bs_scan(cnt, nseg, bsum, rule_ptr, s);
    sq_eval_kernel<true><<<tgrid, BS_THREADS, 0, s>>>(keys, pos, start, occ, l.table, cap, shift, nseg,
                                                       rules.anchor_ptr, rules.anchor_rules, rules.rterm_ptr, rules.recs,
                                                       rules.ngid, rules.nrules, rules.nterms, cnt, rule_ptr, hits,
                                                       hits_cap);
    return hipGetLastError();
}
