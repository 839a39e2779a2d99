// pm_bystream_dev.h -- the device helpers that the per-stream sets
// (pm_bystream.hip) and the rules (pm_rules.hip) share: the number of events
// used, the stream of a position and the hash of a (stream, gid) key.  Device
// code only; every function is inlined into its callers.
#ifndef PM_BYSTREAM_DEV_H
#define PM_BYSTREAM_DEV_H

#include <hip/hip_runtime.h>

#include "pm_bystream.h"

namespace {

constexpr int BS_THREADS = 256;
constexpr uint32_t BS_NO_STREAM = 0xFFFFFFFFu;
constexpr unsigned long long BS_EMPTY = ~0ull;
using u64 = unsigned long long;

__device__ __forceinline__ uint64_t bs_used(const unsigned long long* nevents, uint64_t cap) {
    const uint64_t c = *nevents;
    return c < cap ? c : cap;
}

// The first index i in [lo, cnt] with offs[i] > p (cnt where none is), given
// that every offset before lo is <= p: flow_seek's gallop, then bisection.
// At most 2 log2(cnt) + 2 loads, every index below cnt.
__device__ __forceinline__ int64_t bs_seek(const int64_t* __restrict__ offs, int64_t lo, int64_t cnt, int64_t p) {
    int64_t hi = lo, step = 1;
    while (hi < cnt && offs[hi] <= p) {
        lo = hi + 1;
        hi += step;
        step <<= 1;
    }
    if (hi > cnt) hi = cnt;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (offs[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t bs_first_lane(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The stream of position p: the j with offs[j] <= p < offs[j + 1]
// (BS_NO_STREAM where none holds it, and for a lane without an event).  Called
// by a whole wave.  A list is appended in wave-sized flushes of neighbouring
// tiles, so the wave's events mostly lie in the leader's stream or the next
// few: lane 0's search runs once for the wave (on scalar registers), a lane
// inside its range [lo0, hi0) is done, a lane above it gallops on from there,
// and only a lane below it searches from the start.  [slo, shi) = the found
// stream's positions.
__device__ __forceinline__ uint32_t bs_stream_of(const int64_t* __restrict__ offs, int64_t nseg, int64_t p,
                                                 bool valid, int64_t& slo, int64_t& shi) {
    const int64_t p0 = bs_first_lane(p);  // valid lanes are a prefix of the wave: lane 0 has an event or none has
    int64_t j0 = bs_seek(offs, 0, nseg + 1, p0) - 1;
    j0 = j0 < 0 ? 0 : j0 >= nseg ? nseg - 1 : j0;
    const int64_t lo0 = offs[j0], hi0 = offs[j0 + 1];
    slo = lo0;
    shi = hi0;
    if (!valid) return BS_NO_STREAM;
    int64_t j = j0;
    if (p < lo0 || p >= hi0) {
        j = bs_seek(offs, p >= hi0 ? j0 + 1 : 0, nseg + 1, p) - 1;
        j = j < 0 ? 0 : j >= nseg ? nseg - 1 : j;
        slo = offs[j];
        shi = offs[j + 1];
        if (p < slo || p >= shi) return BS_NO_STREAM;  // outside every stream
    }
    return (uint32_t)j;
}

// The hash of a stream << 24 | gid key: its top bits, 64 - shift of them.
__device__ __forceinline__ uint64_t bs_hash(uint64_t key, int shift) { return (key * 0x9E3779B97F4A7C15ull) >> shift; }

}  // namespace

#endif  // PM_BYSTREAM_DEV_H
