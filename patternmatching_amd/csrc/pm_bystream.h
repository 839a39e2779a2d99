// pm_bystream.h -- per-stream match sets (include/pm_hip.h, "per-stream
// sets"): what the device passes (pm_bystream.hip), their host twin
// (pm_bystream_host.cpp) and the plugin's entry points share.
#ifndef PM_BYSTREAM_H
#define PM_BYSTREAM_H

#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

// An event is position << 24 | gid (pm_hip.h, "match list").
constexpr int PM_BS_GID_BITS = 24;
constexpr uint64_t PM_BS_GID_MASK = (1ull << PM_BS_GID_BITS) - 1;
constexpr uint64_t PM_BS_MAX_CAP = 1ull << 40;
constexpr int64_t PM_BS_MAX_NSEG = (int64_t)1 << 31;  // exclusive
// The scan's block width: one count per thread, so a launch of the block sums
// covers 1,024 streams per workgroup and the middle level 1,024 sums per turn
// of its loop.
constexpr int PM_BS_SCAN_BLOCK = 1024;
constexpr uint64_t PM_BS_TABLE_MIN = 64;  // slots: one wave's worth, so every table pass has whole waves

// The scratch of one call, in this order, each part rounded up to 16 bytes:
//   plain:   sid   u32 x cap      the stream of each event (~0: dropped)
//   UNIQUE:  keys  u64 x T        the hash table's keys, stream << 24 | gid (all-ones: empty)
//            pos   u64 x T        ... the smallest position of each key
//            rank  u32 x T        ... and the key's place in its stream's range
//   both:    cnt   u64 x nseg     events kept per stream; the scatter counts it back down to 0
//            bsum  u64 x ceil(nseg / 1,024)   the scan's block sums
// T = the power of two >= max(2 cap, 64).
struct PmByStreamLayout {
    uint64_t table;  // T (0 in plain mode)
    size_t sid_off, keys_off, pos_off, rank_off, cnt_off, bsum_off;
    size_t bytes;
};

inline size_t pm_bs_round16(size_t b) { return (b + 15) & ~(size_t)15; }

inline uint64_t pm_bs_table_slots(uint64_t cap) {
    uint64_t t = PM_BS_TABLE_MIN;
    while (t < 2 * cap) t <<= 1;
    return t;
}

// cap <= PM_BS_MAX_CAP, 0 <= nseg < PM_BS_MAX_NSEG (the callers check).
inline PmByStreamLayout pm_by_stream_layout(uint64_t cap, int64_t nseg, bool unique) {
    PmByStreamLayout l{};
    size_t at = 0;
    if (unique) {
        l.table = pm_bs_table_slots(cap);
        l.keys_off = at;
        at += (size_t)l.table * sizeof(uint64_t);
        l.pos_off = at;
        at += (size_t)l.table * sizeof(uint64_t);
        l.rank_off = at;
        at += (size_t)l.table * sizeof(uint32_t);
    } else {
        l.sid_off = at;
        at += pm_bs_round16((size_t)cap * sizeof(uint32_t));
    }
    l.cnt_off = at;
    at += pm_bs_round16((size_t)nseg * sizeof(uint64_t));
    l.bsum_off = at;
    const size_t nblk = ((size_t)nseg + PM_BS_SCAN_BLOCK - 1) / PM_BS_SCAN_BLOCK;
    at += pm_bs_round16(nblk * sizeof(uint64_t));
    l.bytes = at;
    return l;
}

// The workgroups of a grid-stride launch over `items` lanes' worth of work:
// 2,048 lanes per CU at the most, the loop beyond.
inline int pm_bs_grid(uint64_t items, int num_cu) {
    const uint64_t want = (items + 255) / 256;
    const uint64_t most = (uint64_t)(num_cu > 0 ? num_cu : 256) * 8;
    return (int)(want < 1 ? 1 : want > most ? most : want);
}

#ifdef __HIPCC__
// The exclusive scan of cnt[0, nseg) into stream_ptr[0, nseg] (stream_ptr[nseg]
// = the sum), three launches on s; bsum holds ceil(nseg / PM_BS_SCAN_BLOCK)
// words.  nseg >= 1.  cnt is left as it is.
void pm_launch_bs_scan(const unsigned long long* cnt, int64_t nseg, unsigned long long* bsum, int64_t* stream_ptr,
                       hipStream_t s);

// The passes of pm_hip_events_by_stream_device, enqueued on s in stream order
// (nseg >= 1, cap >= 1; every pointer checked by the caller; scratch holds
// pm_by_stream_layout(cap, nseg, unique).bytes).  Nothing is allocated and
// the host is never waited for.
hipError_t pm_launch_by_stream(const uint64_t* events, uint64_t cap, const unsigned long long* nevents,
                               const int64_t* offsets, int64_t nseg, bool unique, uint64_t* out, uint64_t out_cap,
                               int64_t* stream_ptr, void* scratch, int num_cu, hipStream_t s);
#endif

#endif  // PM_BYSTREAM_H
