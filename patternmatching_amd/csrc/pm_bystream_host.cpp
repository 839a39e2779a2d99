// pm_bystream_host.cpp -- the host twin of the per-stream sets
// (include/pm_hip.h, "per-stream sets") and the scratch formula.  Plain C++:
// no handle, no device, no HIP.
#include <algorithm>
#include <utility>
#include <vector>

#include "pm_bystream.h"
#include "pm_hip.h"

extern "C" size_t pm_hip_by_stream_scratch_bytes(uint64_t cap, int64_t nseg, uint32_t flags) {
    if (cap > PM_BS_MAX_CAP || nseg < 0 || nseg >= PM_BS_MAX_NSEG || (flags & ~PM_BY_STREAM_UNIQUE)) return (size_t)-1;
    return pm_by_stream_layout(cap, nseg, (flags & PM_BY_STREAM_UNIQUE) != 0).bytes;
}

namespace {

// The stream of position p, or -1: the first offset above p, minus one, when
// that stream holds p.  Bisection over indices alone, so offsets that are not
// sorted give some stream or none and nothing else.
int64_t stream_of(const int64_t* offs, size_t nseg, int64_t p) {
    size_t lo = 0, hi = nseg + 1;
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (offs[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0 || lo > nseg) return -1;
    const size_t j = lo - 1;
    return offs[j] <= p && p < offs[j + 1] ? (int64_t)j : -1;
}

}  // namespace

extern "C" int pm_flat_events_by_stream(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                                        uint32_t flags, uint64_t* out, size_t out_cap, int64_t* stream_ptr) {
    if ((nevents && !events) || (nseg && (!offsets || !stream_ptr)) || (out_cap && !out) ||
        nseg >= (size_t)PM_BS_MAX_NSEG || nevents > PM_BS_MAX_CAP || (flags & ~PM_BY_STREAM_UNIQUE) ||
        (out && out == events))
        return -2;
    if (nseg == 0) return 0;
    const bool unique = (flags & PM_BY_STREAM_UNIQUE) != 0;
    // (stream, event) of every event inside a stream; UNIQUE orders a stream by
    // gid, then position, so the first of each gid is its smallest position
    std::vector<std::pair<uint64_t, uint64_t>> kept;
    kept.reserve(nevents);
    for (size_t k = 0; k < nevents; ++k) {
        const uint64_t ev = events[k];
        const int64_t j = stream_of(offsets, nseg, (int64_t)(ev >> PM_BS_GID_BITS));
        if (j < 0) continue;
        kept.emplace_back((uint64_t)j, unique ? ((ev & PM_BS_GID_MASK) << 40) | (ev >> PM_BS_GID_BITS) : ev);
    }
    std::sort(kept.begin(), kept.end());
    if (unique) {
        size_t w = 0;
        uint64_t last_j = ~0ull, last_gid = ~0ull;  // (slots below w already hold events again)
        for (size_t k = 0; k < kept.size(); ++k) {
            const uint64_t v = kept[k].second;
            if (kept[k].first == last_j && (v >> 40) == last_gid) continue;
            last_j = kept[k].first;
            last_gid = v >> 40;
            kept[w++] = {kept[k].first, ((v & ((1ull << 40) - 1)) << PM_BS_GID_BITS) | (v >> 40)};
        }
        kept.resize(w);
        std::sort(kept.begin(), kept.end());  // each stream's range ascending as plain u64 again
    }
    size_t at = 0;
    for (size_t j = 0; j < nseg; ++j) {
        stream_ptr[j] = (int64_t)at;
        while (at < kept.size() && kept[at].first == j) ++at;
    }
    stream_ptr[nseg] = (int64_t)kept.size();
    const size_t store = std::min(out_cap, kept.size());
    for (size_t k = 0; k < store; ++k) out[k] = kept[k].second;
    return 0;
}
