// pm_bystream.hip -- per-stream match sets on the device (include/pm_hip.h,
// "per-stream sets"): a match list of position << 24 | gid
// events, in any order behind its cursor, becomes per-stream ranges in CSR
// form, optionally with one event per (stream, gid).
//
// Separate launches in stream order; no kernel waits on another workgroup and
// every loop is bounded by a kernel argument:
//   plain:   lookup + count -> scan (3 launches) -> scatter
//   UNIQUE:  lookup + hash insert + count -> scan -> scatter the table
// The number of events used, min(*nevents, cap), is read on the device by
// every pass, so the call can follow a scan with no synchronize between.
//
// Memory safety does not depend on the data: a stream index is clamped into
// [0, nseg) before any offsets[j] / offsets[j + 1] and is the only index into
// cnt and stream_ptr; the count and the scatter read the same stream index
// per event (sid), so a stream's cursor never passes its count; a slot is
// stored only below out_cap; a probe index is masked by the table size.
#include <hip/hip_runtime.h>

#include "pm_bystream.h"
#include "pm_bystream_dev.h"

namespace {

// Runs of equal stream indices among a wave's neighbouring lanes: a lane is a
// head where its left neighbour's index differs (lane 0 always).  Returns the
// lane of this lane's head; len = the run's length, meaningful at a head.
__device__ __forceinline__ int bs_runs(uint32_t j, int lane, bool& head, int& len) {
    const uint32_t left = __shfl_up(j, 1);
    head = lane == 0 || left != j;
    const uint64_t heads = __ballot(head);
    const uint64_t upto = heads & (~0ull >> (63 - lane));  // heads at or below this lane: never empty (lane 0)
    const int hlane = 63 - __clzll((long long)upto);
    const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
    len = above ? __ffsll((long long)above) : 64 - lane;
    return hlane;
}

// ---- plain mode ---------------------------------------------------------------
// Pass 1: the stream of every used event to sid, and the streams' counts: a
// run's head adds the run's length (one atomic per run, none returning).
__global__ void __launch_bounds__(BS_THREADS)
bs_lookup_count_kernel(const uint64_t* __restrict__ events, uint64_t cap, const unsigned long long* __restrict__ nevents,
                       const int64_t* __restrict__ offs, int64_t nseg, uint32_t* __restrict__ sid,
                       u64* __restrict__ cnt) {
    const uint64_t used = bs_used(nevents, cap);
    const uint64_t rounded = (used + 63) & ~63ull;  // whole waves take every turn of the loop
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    const int lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < rounded; i += stride) {
        const bool valid = i < used;
        const uint64_t ev = valid ? events[i] : 0;
        int64_t slo, shi;
        const uint32_t j = bs_stream_of(offs, nseg, (int64_t)(ev >> PM_BS_GID_BITS), valid, slo, shi);
        if (valid) sid[i] = j;
        bool head;
        int len;
        (void)bs_runs(j, lane, head, len);
        if (head && j != BS_NO_STREAM) atomicAdd(&cnt[j], (u64)len);
    }
}

// ---- UNIQUE: the hash table -------------------------------------------------------
// Pass 1: every used event that lies in a stream claims the slot of its key
// stream << 24 | gid (64-bit compare-and-swap on an empty slot; linear
// probing, at most max_probe = the table's slots steps) and folds its position
// into the slot's minimum.  Both words only ever move one way (empty -> key,
// position downwards), so a plain look before each atomic can only skip an
// atomic that would change nothing: 4,096 events of one key cost one
// compare-and-swap and a handful of minima, not 8,192 atomics on two words.
// The table has at least twice as many slots as the call has events, so a
// probe sequence always ends at the key or at an empty slot.
// Exactly one lane claims a key.  The claimers also count: the list is in
// stream order, more or less, so a wave's claimers lie in a few streams; per
// such stream one lane adds their number to the stream's count and hands the
// old value round, and each claimer keeps it plus its place among them as the
// key's rank in its stream -- stored beside the slot, so the scatter needs no
// cursor.  (Counting and ranking the occupied slots in two passes over the
// table meets them in hash order, where no two neighbours share a stream:
// DESIGN.md §4.)
__global__ void __launch_bounds__(BS_THREADS)
bs_insert_kernel(const uint64_t* __restrict__ events, uint64_t cap, const unsigned long long* __restrict__ nevents,
                 const int64_t* __restrict__ offs, int64_t nseg, u64* keys, u64* pos, uint32_t* __restrict__ rank,
                 u64* __restrict__ cnt, uint64_t mask, int shift, uint64_t max_probe) {
    const uint64_t used = bs_used(nevents, cap);
    const uint64_t rounded = (used + 63) & ~63ull;
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    const int lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < rounded; i += stride) {
        const bool valid = i < used;
        const uint64_t ev = valid ? events[i] : 0;
        const uint64_t p = ev >> PM_BS_GID_BITS;
        int64_t slo, shi;
        const uint32_t j = bs_stream_of(offs, nseg, (int64_t)p, valid, slo, shi);
        const u64 key = ((u64)j << PM_BS_GID_BITS) | (ev & PM_BS_GID_MASK);
        uint64_t h = bs_hash(key, shift) & mask;
        bool found = false, claimed = false;
        for (uint64_t probe = 0; j != BS_NO_STREAM && probe < max_probe; ++probe) {
            u64 k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == BS_EMPTY) {
                k = atomicCAS(&keys[h], BS_EMPTY, key);
                if (k == BS_EMPTY) {
                    k = key;
                    claimed = true;
                }
            }
            if (k == key) {
                found = true;
                break;
            }
            h = (h + 1) & mask;
        }
        if (found && __hip_atomic_load(&pos[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > p) atomicMin(&pos[h], (u64)p);
        // the claimers' counts and ranks: one turn per stream among them, 64 at the most
        uint64_t pending = __ballot(claimed);
        uint32_t r = 0;
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const uint32_t jl = __shfl(j, leader);  // < nseg: a claimer's stream
            const bool mine = claimed && j == jl;
            const uint64_t same = __ballot(mine);
            u64 base = 0;
            if (lane == leader) base = atomicAdd(&cnt[jl], (u64)__popcll(same));
            base = (u64)__shfl((long long)base, leader);
            if (mine) r = (uint32_t)(base + (u64)__popcll(same & ((1ull << lane) - 1)));
            pending &= ~same;
        }
        if (claimed) rank[h] = r;
    }
}

// ---- scatter -----------------------------------------------------------------------
// Plain mode's last pass: a run's head takes the run's slots from its stream's
// count (counted back down: the streams' counts are the cursors, and end at
// 0), the run's lanes store behind stream_ptr[j], below out_cap only.
__global__ void __launch_bounds__(BS_THREADS)
bs_scatter_kernel(const uint64_t* __restrict__ events, uint64_t cap, const unsigned long long* __restrict__ nevents,
                  const uint32_t* __restrict__ sid, int64_t nseg, const int64_t* __restrict__ stream_ptr,
                  u64* __restrict__ cnt, uint64_t* __restrict__ out, uint64_t out_cap) {
    const uint64_t used = bs_used(nevents, cap);
    const uint64_t rounded = (used + 63) & ~63ull;
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    const int lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < rounded; i += stride) {
        const bool valid = i < used;
        const uint64_t ev = valid ? events[i] : 0;
        uint32_t j = valid ? sid[i] : BS_NO_STREAM;
        if ((int64_t)j >= nseg) j = BS_NO_STREAM;
        bool head;
        int len;
        const int hlane = bs_runs(j, lane, head, len);
        u64 base = 0;
        if (head && j != BS_NO_STREAM) base = atomicAdd(&cnt[j], (u64)0 - (u64)len) - (u64)len;
        base = (u64)__shfl((long long)base, hlane);
        if (j != BS_NO_STREAM) {
            const uint64_t slot = (uint64_t)stream_ptr[j] + base + (uint64_t)(lane - hlane);
            if (slot < out_cap) out[slot] = ev;
        }
    }
}

// UNIQUE's last pass: an occupied slot's event goes to its rank behind
// stream_ptr[j], below out_cap only; no atomics.
__global__ void __launch_bounds__(BS_THREADS)
bs_table_scatter_kernel(const u64* __restrict__ keys, const u64* __restrict__ pos, const uint32_t* __restrict__ rank,
                        uint64_t table, int64_t nseg, const int64_t* __restrict__ stream_ptr,
                        uint64_t* __restrict__ out, uint64_t out_cap) {
    const uint64_t stride = (uint64_t)gridDim.x * BS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x; i < table; i += stride) {
        const u64 k = keys[i];
        if (k == BS_EMPTY) continue;
        const u64 j = k >> PM_BS_GID_BITS;
        if (j >= (u64)nseg) continue;
        const uint64_t slot = (uint64_t)stream_ptr[j] + rank[i];
        if (slot < out_cap) out[slot] = (pos[i] << PM_BS_GID_BITS) | (k & PM_BS_GID_MASK);
    }
}

// ---- the exclusive scan of the counts ---------------------------------------------
// One value per thread of a PM_BS_SCAN_BLOCK-wide workgroup: the sum of the
// values of the threads before this one; total = the workgroup's sum.  lds: 16
// words.  Ends with every thread past its last read of lds.
__device__ __forceinline__ u64 bs_block_scan(u64 v, u64* lds, u64& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 t = (u64)__shfl_up((long long)x, d);
        if (lane >= d) x += t;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    u64 before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < PM_BS_SCAN_BLOCK / 64; ++w) {
        const u64 s = lds[w];
        if (w < wave) before += s;
        all += s;
    }
    __syncthreads();
    total = all;
    return before + x - v;
}

// Level 1: bsum[b] = the sum of block b's counts.
__global__ void __launch_bounds__(PM_BS_SCAN_BLOCK)
bs_scan_sums_kernel(const u64* __restrict__ cnt, int64_t nseg, u64* __restrict__ bsum) {
    __shared__ u64 lds[PM_BS_SCAN_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * PM_BS_SCAN_BLOCK + threadIdx.x;
    u64 total;
    (void)bs_block_scan(i < nseg ? cnt[i] : 0, lds, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// Level 2, one workgroup: bsum becomes its own exclusive scan, 1,024 sums per
// turn with the carry in a register (nblk turns / 1,024: no size limit), and
// stream_ptr[nseg] the number of events kept.
__global__ void __launch_bounds__(PM_BS_SCAN_BLOCK)
bs_scan_middle_kernel(u64* __restrict__ bsum, int64_t nblk, int64_t* __restrict__ stream_ptr, int64_t nseg) {
    __shared__ u64 lds[PM_BS_SCAN_BLOCK / 64];
    u64 carry = 0;
    for (int64_t base = 0; base < nblk; base += PM_BS_SCAN_BLOCK) {
        const int64_t i = base + threadIdx.x;
        u64 total;
        const u64 ex = bs_block_scan(i < nblk ? bsum[i] : 0, lds, total);
        if (i < nblk) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) stream_ptr[nseg] = (int64_t)carry;
}

// Level 3: stream_ptr[j] = the events kept in the streams before j.
__global__ void __launch_bounds__(PM_BS_SCAN_BLOCK)
bs_scan_add_kernel(const u64* __restrict__ cnt, int64_t nseg, const u64* __restrict__ bsum,
                   int64_t* __restrict__ stream_ptr) {
    __shared__ u64 lds[PM_BS_SCAN_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * PM_BS_SCAN_BLOCK + threadIdx.x;
    u64 total;
    const u64 ex = bs_block_scan(i < nseg ? cnt[i] : 0, lds, total);
    if (i < nseg) stream_ptr[i] = (int64_t)(bsum[blockIdx.x] + ex);
}

}  // namespace

void pm_launch_bs_scan(const unsigned long long* cnt, int64_t nseg, unsigned long long* bsum, int64_t* stream_ptr,
                       hipStream_t s) {
    const int64_t nblk = (nseg + PM_BS_SCAN_BLOCK - 1) / PM_BS_SCAN_BLOCK;
    bs_scan_sums_kernel<<<(unsigned)nblk, PM_BS_SCAN_BLOCK, 0, s>>>(cnt, nseg, bsum);
    bs_scan_middle_kernel<<<1, PM_BS_SCAN_BLOCK, 0, s>>>(bsum, nblk, stream_ptr, nseg);
    bs_scan_add_kernel<<<(unsigned)nblk, PM_BS_SCAN_BLOCK, 0, s>>>(cnt, nseg, bsum, stream_ptr);
}

hipError_t pm_launch_by_stream(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                               const int64_t* offsets, int64_t nseg, bool unique, uint64_t* out, uint64_t out_cap,
                               int64_t* stream_ptr, void* scratch, int num_cu, hipStream_t s) {
    const PmByStreamLayout l = pm_by_stream_layout(cap, nseg, unique);
    char* base = (char*)scratch;
    uint32_t* sid = (uint32_t*)(base + l.sid_off);
    u64* keys = (u64*)(base + l.keys_off);
    u64* pos = (u64*)(base + l.pos_off);
    uint32_t* rank = (uint32_t*)(base + l.rank_off);
    u64* cnt = (u64*)(base + l.cnt_off);
    u64* bsum = (u64*)(base + l.bsum_off);
    hipError_t e = hipMemsetAsync(cnt, 0, (size_t)nseg * sizeof(u64), s);
    if (e != hipSuccess) return e;
    const int egrid = pm_bs_grid(cap, num_cu);
    if (unique) {
        // keys and pos lie back to back: one fill empties both
        e = hipMemsetAsync(keys, 0xFF, 2 * (size_t)l.table * sizeof(u64), s);
        if (e != hipSuccess) return e;
        int shift = 64;
        for (uint64_t t = l.table; t > 1; t >>= 1) --shift;
        bs_insert_kernel<<<egrid, BS_THREADS, 0, s>>>(events, cap, nevents, offsets, nseg, keys, pos, rank, cnt,
                                                       l.table - 1, shift, l.table);
    } else {
        bs_lookup_count_kernel<<<egrid, BS_THREADS, 0, s>>>(events, cap, nevents, offsets, nseg, sid, cnt);
    }
    pm_launch_bs_scan(cnt, nseg, bsum, stream_ptr, s);
    if (unique)
        bs_table_scatter_kernel<<<pm_bs_grid(l.table, num_cu), BS_THREADS, 0, s>>>(keys, pos, rank, l.table, nseg,
                                                                                    stream_ptr, out, out_cap);
    else
        bs_scatter_kernel<<<egrid, BS_THREADS, 0, s>>>(events, cap, nevents, sid, nseg, stream_ptr, cnt, out, out_cap);
    return hipGetLastError();
}
