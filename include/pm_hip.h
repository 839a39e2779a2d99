/*
 * pm_hip.h -- C-ABI of the MI355X (gfx950) matcher library libpm.so.
 *
 * Two groups of entry points:
 *
 * 1. The plugin functions behind pm_mps_table (include/pm_mps.h).  Each one
 *    replaces the reference function named beside it, with the same
 *    argument meaning and the same "no error channel" behaviour: a HIP
 *    failure prints a message and exits(1), like FatalExit()
 *    (/root/reference/Core/src/util.h:37-39).
 *
 *      reference (Core/src/)            this library
 *      mpac.c:236  ac_create            pm_hip_rt_create / pm_hip_ac_create
 *      mpac.c:257  ac_add_pattern       pm_hip_add_pattern
 *      mpac.c:282  ac_compile           pm_hip_compile
 *      mpac.c:304  ac_read_char         pm_hip_read_char
 *      (none)                           pm_hip_read_block (batched read_char)
 *      mpac.c:328  ac_total_mem         pm_hip_total_mem
 *      mpac.c:339  ac_reset             pm_hip_reset
 *      mpac.c:349  ac_free              pm_hip_free
 *      mpac.c:358  mps_ac_register      pm_mps_hip_rt_register / pm_mps_hip_ac_register
 *
 *    The same functions serve both algorithms; the object created decides
 *    which kernel runs.
 *
 * 2. Device-resident batch entry points for callers that keep the stream in
 *    HBM (bench.py, the multi-GPU driver).  They return 0 on success and a
 *    negative code on failure (message via pm_hip_last_error()).
 *
 * Pattern ids inside the library are "gids": 1..n_patterns, 0 = no match.
 * pm_hip_gid_index maps a gid back to the 0-based add_pattern call order.
 */
#ifndef PM_HIP_H
#define PM_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "pm_mps.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. plugin ABI (MpsElem members) ---------------------------------- */
void* pm_hip_rt_create(void);
void* pm_hip_ac_create(void);
/* Both kernels; each launch picks one: the RT kernel, unless the last RT
 * launch spilled more than 10% of its positions (dense deep matches), when
 * the next 64 launches run the AC-DFA kernel.  reset()
 * forgets the choice. */
void* pm_hip_auto_create(void);
void pm_hip_add_pattern(void* obj, char* pat, size_t len, pm_pattern_id_t id);
void pm_hip_compile(void* obj);
pm_pattern_id_t pm_hip_read_char(void* obj, char c);
void pm_hip_read_block(void* obj, const char* buf, size_t n, pm_pattern_id_t* out);
size_t pm_hip_total_mem(void* obj);
void pm_hip_reset(void* obj);
void pm_hip_free(void* obj);

void pm_mps_hip_rt_register(PmMpsElem* slot);
void pm_mps_hip_ac_register(PmMpsElem* slot);
void pm_mps_hip_auto_register(PmMpsElem* slot);

/* ---- 2. batch / introspection ----------------------------------------- */

/* Same as pm_hip_read_block but writes gids (u32, 0 = none) instead of
 * pattern ids; state carries across calls exactly like read_block. */
int pm_hip_read_block_gid(void* obj, const uint8_t* buf, size_t n, uint32_t* out_gid);

/*
 * Scan positions [pos0, pos0+n) of the device buffer d_text.
 *   stream_start  index in d_text of the stream's first byte (<= pos0);
 *                 bytes in [stream_start, pos0) are context: they are looked
 *                 back at but produce no output.  Context of
 *                 pm_hip_max_pattern_len()-1 bytes makes the result exact for
 *                 a position anywhere in a longer stream.
 *   pos0          must be a multiple of 16; d_text 16-byte aligned and
 *                 readable up to round_up(pos0+n, 16).
 *   d_out         n u32 gids (16-byte aligned), or NULL for count-only.
 *   d_count       device u64, incremented by the number of non-null
 *                 positions (may be NULL).
 *   hip_stream    hipStream_t to launch on (NULL = default stream).
 * Asynchronous: returns after the launch.
 */
int pm_hip_scan_device(void* obj, const uint8_t* d_text, int64_t stream_start, int64_t pos0,
                       int64_t n, uint32_t* d_out, unsigned long long* d_count, void* hip_stream);
/* The same with u16 gids (n * 2 bytes, 16-byte aligned): the compact id
 * stream for dictionaries of fewer than 65536 patterns (every reference
 * dictionary; the merged snort + ET set has 55,580).  Returns -4 when the
 * dictionary is larger. */
int pm_hip_scan_device16(void* obj, const uint8_t* d_text, int64_t stream_start, int64_t pos0,
                         int64_t n, uint16_t* d_out, unsigned long long* d_count, void* hip_stream);

/*
 * Batched scan: nseg independent streams (packets, flows, small files, log
 * lines) in one launch.  The streams lie back to back in one buffer of n
 * bytes; offsets has nseg + 1 non-decreasing int64 values with offsets[0] ==
 * 0 and offsets[nseg] == n, and stream j is bytes [offsets[j], offsets[j+1]).
 * Empty streams, and runs of them, are legal.  The answer at position i of
 * stream j is what read_char returns after reset() and the stream's bytes up
 * to and including i (mpac.c:304-319 from the root state): the reset at a new
 * stream file of the reference's loop (measure.c:241-311), once per stream
 * inside one call.  Output is dense, n ids in buffer order: stream j's
 * answers are d_out[offsets[j] .. offsets[j+1]).
 *   d_text      device buffer, 16-byte aligned, n bytes.
 *   d_offsets   DEVICE pointer, 8-byte aligned, nseg + 1 values.  The device
 *               form does not check them: offsets that are not sorted, or do
 *               not end at n, give unspecified ids, but never a read outside
 *               d_text[0, round_up(n, 16)) or a write outside d_out[0, n).
 *   d_out       n u32 gids (16-byte aligned), or NULL for count only.
 *   d_count     device u64 += non-null positions (may be NULL).
 * Asynchronous, on hip_stream; needs no scratch and allocates nothing, so it
 * may be captured into a graph without pm_hip_prepare_capture.  Like
 * pm_hip_scan_device it asks the resident read_block server to leave the
 * device first.  nseg == 0 or n == 0: returns 0, launches nothing.
 * Returns 0, -1 before compile(), -2 bad arguments (negative nseg or n,
 * alignment), -3 launch error, and
 *   -6  the object holds no reverse-trie image: the ac kind, and an rt / auto
 *       object whose dictionary compile() gave to the DFA because the
 *       reverse-trie encoding did not hold it.  The batched scan is the
 *       reverse-trie walk with a stream start per position; the segmented DFA
 *       walk is the flow scan below (pm_hip_scan_flows_device), which those
 *       objects run.  Nothing is launched, d_out is untouched and
 *       pm_hip_last_error says why.
 * Launches of at most "rt_small_max" positions run one thread per position
 * over the global tables, larger ones one workgroup per CU (DESIGN.md §4,
 * rt_batch_kernel).
 */
int pm_hip_scan_batch_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                             int64_t n, uint32_t* d_out, unsigned long long* d_count, void* hip_stream);
/* The same with u16 gids; -4 above 65,535 patterns, as pm_hip_scan_device16. */
int pm_hip_scan_batch_device16(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                               int64_t n, uint16_t* d_out, unsigned long long* d_count, void* hip_stream);
/* Host forms: buf holds the streams back to back, offsets is a HOST array of
 * nseg + 1 values, checked here (offsets[0] == 0, non-decreasing: else -2);
 * n = offsets[nseg].  Text and offsets are copied to device staging the
 * object keeps (counted in pm_hip_scratch_bytes; plain copies from pageable
 * memory, not read_block's pinned pool), one batch launch, the ids copied
 * back, one synchronize.  out_gid: n u32 gids; pm_hip_read_batch maps them to
 * the add_pattern ids as pm_hip_read_block does.  They neither read nor
 * change what read_block / read_char carry across calls: a batch call in the
 * middle of a stream is invisible to that stream.  Codes as above (-6 too). */
int pm_hip_read_batch_gid(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg, uint32_t* out_gid);
int pm_hip_read_batch(void* obj, const char* buf, const int64_t* offsets, size_t nseg, pm_pattern_id_t* out);

/*
 * Flow scan: the batched layout with a carried state per stream, for flows
 * whose bytes arrive a packet at a time among thousands of other flows.
 * Text, offsets and output are exactly pm_hip_scan_batch_device's; each
 * stream also brings a u32 state in and leaves one out.  A flow state is
 * opaque: 0 means "at the start of a stream", any other value is one this
 * object returned earlier for that flow.  The answer at position i of stream
 * j is what read_char returns after reset(), every byte the flow had in
 * earlier calls, and this call's bytes up to and including i (mpac.c:304-319:
 * the automaton state kept across chunks, reset only at a new stream file,
 * measure.c:241-311) -- so a pattern that straddles a packet boundary is
 * found, which a batch call per packet misses.
 *   d_state_in   DEVICE pointer, 4-byte aligned, nseg values, or NULL: every
 *                stream fresh.  The device form does not check the values: a
 *                state >= pm_hip_flow_states(obj) is used as 0.
 *   d_state_out  DEVICE pointer, 4-byte aligned, nseg values, or NULL:
 *                d_state_out[j] = the state after stream j's last byte; for
 *                an empty stream the state it came in with.  Must not overlap
 *                d_state_in (one lane reads state_in[j] while another writes
 *                state_out[j]): callers ping-pong two arrays.
 * A flow appears at most once per call (its state would be read once and
 * written twice): a caller holding two packets of one flow concatenates them
 * into one stream.  The walk runs over the DFA's dense rows (dfa_flow_kernel,
 * DESIGN.md §4); on the DFA a flow's whole history is this one u32.
 * Asynchronous, on hip_stream; needs no scratch and allocates nothing, so it
 * may be captured into a graph.  It asks the resident read_block server to
 * leave the device first, reads and changes nothing read_block / read_char
 * carry, and leaves the auto kind's kernel pick alone.  Afterwards
 * pm_hip_kernel_last is 2 and pm_hip_dfa_form_last is 1.
 * nseg == 0: returns 0, launches nothing, the state arrays are untouched.
 * n == 0 with nseg > 0: every stream is empty; the kernel's state-copy pass
 * alone is launched (d_state_out[j] = d_state_in[j]), nothing when
 * d_state_out is NULL.
 * Returns 0, -1 before compile(), -2 bad arguments (negative nseg or n;
 * alignment: text and ids 16 B, offsets 8 B, states 4 B; d_state_in ==
 * d_state_out), -3 launch error, -4 u16 ids above 65,535 patterns, and
 *   -6  the object holds no DFA image (the rt kind): nothing is launched or
 *       written and pm_hip_last_error names the ac / auto kinds.
 * The "flow_seg" option forces the lane segment length (tests, A/B timing).
 */
int pm_hip_scan_flows_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg, int64_t n,
                             const uint32_t* d_state_in, uint32_t* d_state_out, uint32_t* d_out,
                             unsigned long long* d_count, void* hip_stream);
/* The same with u16 gids; -4 above 65,535 patterns, as pm_hip_scan_device16. */
int pm_hip_scan_flows_device16(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg, int64_t n,
                               const uint32_t* d_state_in, uint32_t* d_state_out, uint16_t* d_out,
                               unsigned long long* d_count, void* hip_stream);
/* Host forms, as pm_hip_read_batch*: buf, offsets and state are HOST arrays;
 * offsets is checked (offsets[0] == 0, non-decreasing) and so is every state
 * (< pm_hip_flow_states), else -2 with nothing written.  state: nseg values,
 * read as the streams' states in and overwritten with their states out (the
 * call copies, so one array serves both), or NULL: every stream fresh and no
 * state returned.  Text, offsets and ids use the batch calls' staging, the
 * states two device buffers beside it (all in pm_hip_scratch_bytes); one flow
 * launch, one synchronize.  n == 0: every stream keeps its state, so nothing
 * is copied or launched.  pm_hip_read_flows maps the gids to the add_pattern
 * ids as pm_hip_read_block does.  Codes as above (-6 too). */
int pm_hip_read_flows_gid(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg, uint32_t* state,
                          uint32_t* out_gid);
int pm_hip_read_flows(void* obj, const char* buf, const int64_t* offsets, size_t nseg, uint32_t* state,
                      pm_pattern_id_t* out);
/* Flow states of the object: valid states are 0 .. this - 1; 0 before
 * compile() and without a DFA image (the rt kind). */
uint32_t pm_hip_flow_states(void* obj);

/*
 * Match list: the batched and the flow scan with a compacted output for
 * callers that want the few positions where a real pattern ends, not an id
 * per byte (an IDS over packets, flows or log lines; dictionaries with 1- and
 * 2-byte patterns answer 92-99% of all positions).  An event is one uint64_t,
 * position << 24 | gid: the position is an index into the call's buffer, as
 * for the dense outputs, so plain u64 order is position order, and there is
 * at most one event per position.  Position i emits an event iff its answer
 * g != 0 and pm_hip_pattern_len(g) >= min_len.  The answer is the longest
 * pattern ending at i, so this is "some pattern of at least min_len bytes
 * ends here" and the filter loses nothing for that question (WHICH patterns
 * end there: the all-matches forms below); with min_len >= 3 the patterns of
 * <= 2 bytes, whose gids come first, are rejected by one compare.
 * Text, offsets and states mean exactly what they mean in
 * pm_hip_scan_batch_device / pm_hip_scan_flows_device, with the same memory
 * safety whatever the offsets hold; with nseg == 1 the calls serve a plain
 * stream, for every kind between them.
 *   min_len     >= 1.
 *   d_events    DEVICE pointer, 8-byte aligned, cap events; NULL with cap == 0
 *               for a count only.
 *   d_nevents   DEVICE u64, required: the list's cursor.  Each event takes the
 *               next slot from it (atomicAdd, reserved by a wave for many
 *               events at a time) and is stored only when the slot is below
 *               cap.  After the call it holds its old value plus ALL events
 *               found: the caller zeroes it for a fresh list, or leaves it
 *               and the call appends to an earlier list.  A value above cap
 *               means the list was cut short; which events were kept is then
 *               unspecified, and nothing at or beyond d_events[cap] is written.
 * Order in the list is unspecified.  Asynchronous, on hip_stream; allocates
 * nothing (the u32 length per gid is uploaded by compile() and counted in
 * pm_hip_table_bytes), so the calls may be captured into a graph.  Like their
 * dense siblings they ask the resident read_block server to leave the device
 * first, and pm_hip_kernel_last / pm_hip_dfa_form_last read afterwards as
 * after those.  nseg == 0: returns 0, launches nothing.  n == 0 with
 * nseg > 0: the flow form's state-copy pass alone, as pm_hip_scan_flows_device.
 * Returns 0, and as the dense siblings -1 before compile(), -2 bad arguments
 * (theirs, and min_len == 0, d_nevents NULL, d_events misaligned or NULL with
 * cap > 0, n > 2^40), -3 launch error, -6 the kind without the needed image
 * (batch: ac; flows: rt), and -4 when the dictionary has 2^24 or more patterns.
 * Measured (64 MiB, profiles/events/): on random ASCII (an event per 1,000
 * bytes at min_len 3) the calls take 0.77-0.94x the time of their dense u32
 * siblings.  Where such matches are dense (the lines stream: an event per 6-7
 * bytes, 8 B each) they take 0.98-1.08x and hand back as many bytes: a caller
 * with match-dense input keeps the ids.
 */
int pm_hip_scan_batch_events_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                                    int64_t n, uint32_t min_len, uint64_t* d_events, uint64_t cap,
                                    unsigned long long* d_nevents, void* hip_stream);
int pm_hip_scan_flows_events_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                                    int64_t n, const uint32_t* d_state_in, uint32_t* d_state_out, uint32_t min_len,
                                    uint64_t* d_events, uint64_t cap, unsigned long long* d_nevents,
                                    void* hip_stream);
/* Bytes of pattern gid; 0 when out of range (gid 0 too) and before compile(). */
uint32_t pm_hip_pattern_len(void* obj, uint32_t gid);
/* Host forms, as pm_hip_read_batch_gid / pm_hip_read_flows_gid: buf, offsets
 * and state are HOST arrays, validated as there (-2, nothing written), with
 * the same staging plus an events buffer (all in pm_hip_scratch_bytes).
 * *nevents = the total found; events gets the first min(cap, total) of them
 * in ascending position order (the host form sorts).  The device list has to
 * be complete for that: the first launch gives it max(1024, n / 16) events
 * (the "events_cap" option overrides it), and a launch that finds more is
 * repeated once with room for all of them, from the same input states -- they
 * come in and leave through two device arrays.  The states written back are
 * those of the complete scan.  Only the events come back over the link, not
 * 4 n bytes of ids. */
int pm_hip_read_batch_events(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg, uint32_t min_len,
                             uint64_t* events, size_t cap, size_t* nevents);
int pm_hip_read_flows_events(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg, uint32_t* state,
                             uint32_t min_len, uint64_t* events, size_t cap, size_t* nevents);

/*
 * All matches: the match list with an event for EVERY pattern that ends at a
 * position, not only the longest.  The events forms above follow read_char's
 * contract (one answer per position); their filter loses nothing for "does
 * some pattern of at least min_len bytes end here", but a caller that keys a
 * rule on each pattern also needs the shorter ones: with "/admin" and "admin"
 * in the dictionary, a position where "/admin" ends is also one where "admin"
 * ends.  Every pattern ending at i is a suffix of the answer g, so it lies on
 * g's suffix chain g, parent[g], parent[parent[g]], ... (pm_hip_parent_gid;
 * the patterns tree of PatternsTree.c).  Position i emits one event
 * i << 24 | h for every h on that chain with pm_hip_pattern_len(h) >= min_len.
 * Lengths fall strictly along the chain, so these are its first members.
 * The device forms have the arguments, return codes, alignment rules, memory
 * safety, serve_stop behaviour, nseg == 0 / n == 0 cases and
 * pm_hip_kernel_last / pm_hip_dfa_form_last values of
 * pm_hip_scan_batch_events_device / pm_hip_scan_flows_events_device, allocate
 * nothing and may be captured.  They differ in the list alone: a position may
 * bring several events, *d_nevents grows by all of them, and the total may
 * exceed n (chains of up to pm_flat_array("depth")'s maximum: 17-24 in the
 * shipped dictionaries).  So size cap from a count-only call (cap == 0,
 * d_events == NULL) or from a bound such as n times the largest depth, not
 * from n.  Order in the device list is unspecified.
 * The host forms behave like pm_hip_read_*_events (same staging, first launch
 * max(1024, n / 16) slots or "events_cap", one relaunch from the same input
 * states when the list was short, states written back from the complete
 * scan); the list is sorted ascending as plain u64: by position, then by gid
 * within a position (NOT by length: gid order is pm_assign_gids').
 * Measured (64 MiB, min_len 3, profiles/matches/): on random ASCII, where
 * chains are rare (the list grows 1.003-1.004x), the calls take 0.79-0.93x
 * the time of their dense u32 siblings and 0.95-1.03x that of the events
 * forms.  On the lines stream the list grows 1.5-1.6x (an event per 4 bytes,
 * 8 B each) and the calls take 1.04-1.05x (batch) and 1.6-1.9x (flows) the
 * dense call: a caller with match-dense input gains no device time over the
 * ids, only the host walk over the parents (pm_flat_expand_matches does that
 * walk on the host for a caller that keeps the ids).
 */
int pm_hip_scan_batch_matches_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                                     int64_t n, uint32_t min_len, uint64_t* d_events, uint64_t cap,
                                     unsigned long long* d_nevents, void* hip_stream);
int pm_hip_scan_flows_matches_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                                     int64_t n, const uint32_t* d_state_in, uint32_t* d_state_out, uint32_t min_len,
                                     uint64_t* d_events, uint64_t cap, unsigned long long* d_nevents,
                                     void* hip_stream);
int pm_hip_read_batch_matches(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg, uint32_t min_len,
                              uint64_t* events, size_t cap, size_t* nevents);
int pm_hip_read_flows_matches(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg, uint32_t* state,
                              uint32_t min_len, uint64_t* events, size_t cap, size_t* nevents);

/*
 * Pattern groups: one merged automaton, a group mask per pattern and one per
 * stream.  A rule engine gives each packet a subset of the patterns by
 * protocol, direction and port (Snort's port groups, Suricata's
 * signature-group heads); here every pattern has a uint32_t mask, bit k =
 * "member of group k", every stream of a batched or flow call brings the mask
 * of the groups it is scanned for, and pattern h is VISIBLE to stream j iff
 * groups[h] & stream_groups[j] != 0.  The filter runs in the kernel, beside
 * the min_len filter.
 *   all != 0: position i of stream j emits one event i << 24 | h for every
 *     pattern h that ends at i, is visible to j and has at least min_len
 *     bytes: the all-matches list with the invisible patterns removed.
 *   all == 0: at most one event per position, the longest visible pattern of
 *     at least min_len bytes that ends at i -- what a matcher compiled from
 *     the visible patterns alone answers at i (then the min_len test).  This is
 *     NOT the events list filtered by the mask: where the whole dictionary's
 *     answer is invisible, a shorter visible pattern on its suffix chain
 *     (pm_hip_parent_gid) is reported.
 * pm_hip_set_groups(obj, groups, n): groups[k] is the mask of the k-th
 * add_pattern call, n the number of patterns added.  Call it after compile()
 * (-1 before; -2 for a wrong n or NULL groups).  A byte string added twice has
 * the mask of the add that wins (the later one).  The first call allocates two
 * u32 tables of n + 1 entries on the device, which count in
 * pm_hip_table_bytes from then on; a later call overwrites them in place
 * after a device synchronize -- a rule reload: the caller must have no group
 * scan in flight.  compile() allocates nothing for groups, the compiled-image
 * cache does not see them, and an object that never calls it behaves exactly
 * as before.  pm_hip_pattern_groups(obj, gid): the pattern's mask, 0 out of
 * range or before pm_hip_set_groups.
 * The scan calls are pm_hip_scan_batch_matches_device /
 * pm_hip_scan_flows_matches_device with two more arguments: d_stream_groups,
 * a DEVICE pointer to nseg masks, 4-byte aligned, NULL = every stream
 * 0xFFFFFFFF; and all.  The stream index a mask is read at is clamped into
 * [0, nseg), so no mask is read out of bounds whatever the offsets hold.
 * Flow states do not depend on the masks: two calls that differ only in them
 * leave identical d_state_out.  Return codes, alignment rules, memory
 * safety, serve_stop behaviour, the cursor and cap rules, the nseg == 0 /
 * n == 0 cases and pm_hip_kernel_last / pm_hip_dfa_form_last are the
 * siblings'; in addition -7: pm_hip_set_groups was not called (nothing is
 * launched or written, pm_hip_last_error says so).  The calls allocate
 * nothing and may be captured.  Order in the device list is unspecified.
 * The host forms behave like pm_hip_read_*_matches (same staging plus nseg
 * masks, "events_cap", one relaunch when the list was short, the list sorted
 * ascending as plain u64, states written back from the complete scan, -2 with
 * nothing written for bad arguments); stream_groups is a HOST pointer here,
 * NULL = every stream 0xFFFFFFFF.
 * Measured (64 MiB, min_len 3, all form, profiles/groups/): on random ASCII
 * with every stream on all groups the calls take 1.03-1.06x the time of
 * their all-matches siblings (the batched call on 1,500-byte streams
 * 1.055-1.060x, the rest 1.03-1.04x); with each stream on one of 8 disjoint
 * groups 0.98-1.04x.  On the lines stream 1.25-1.49x: every position then
 * loads its stream's mask and two table entries per chain member.
 */
int pm_hip_set_groups(void* obj, const uint32_t* groups, size_t n);
uint32_t pm_hip_pattern_groups(void* obj, uint32_t gid);
int pm_hip_scan_batch_groups_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                                    int64_t n, const uint32_t* d_stream_groups, uint32_t min_len, int all,
                                    uint64_t* d_events, uint64_t cap, unsigned long long* d_nevents,
                                    void* hip_stream);
int pm_hip_scan_flows_groups_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                                    int64_t n, const uint32_t* d_state_in, uint32_t* d_state_out,
                                    const uint32_t* d_stream_groups, uint32_t min_len, int all, uint64_t* d_events,
                                    uint64_t cap, unsigned long long* d_nevents, void* hip_stream);
int pm_hip_read_batch_groups(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg,
                             const uint32_t* stream_groups, uint32_t min_len, int all, uint64_t* events, size_t cap,
                             size_t* nevents);
int pm_hip_read_flows_groups(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg, uint32_t* state,
                             const uint32_t* stream_groups, uint32_t min_len, int all, uint64_t* events, size_t cap,
                             size_t* nevents);

/*
 * Pattern windows: where in its stream a pattern may lie (Snort's and
 * Suricata's `offset` and `depth`), tested for each match inside the scan,
 * beside the group test.  Every pattern k, in add order, has two uint32_t:
 * min_start[k] (`offset`) and max_end[k] (`offset + depth`; 0xFFFFFFFF =
 * unbounded).  Let E be the number of bytes a position's stream has had
 * through position i, this one included: in the batched scan E = i - (the
 * stream's first byte) + 1, in the flow scan E = pos_in[j] + i - offsets[j]
 * + 1.  A pattern h of L bytes that ends at i PASSES ITS WINDOW iff
 * E - L >= min_start[h] and E <= max_end[h], compared in 64 bits (the device
 * compares need = min_start + L and max_end with E saturated to 32 bits,
 * which is the same test: min_start <= 0x7FFFFFFF, L < 2^31).  A window no
 * occurrence can satisfy is legal; the pattern is then never reported.
 * Pattern h is VISIBLE at position i of stream j iff it passes its window
 * there and is group-visible to j exactly as in "pattern groups"; where
 * pm_hip_set_groups was never called every pattern is in every group and
 * d_stream_groups must be NULL (-7 otherwise, as there).
 *   all != 0: one event i << 24 | h for every visible h of at least min_len
 *     bytes that ends at i.
 *   all == 0: at most one event per position, the longest visible pattern of
 *     at least min_len bytes -- the answer of a matcher that knew only the
 *     patterns allowed there.  As with groups this is NOT the events list
 *     filtered: an invisible answer yields to a shorter visible suffix.
 * With windows a short pattern becomes askable: a 2-byte magic anchored at
 * (0, 2) is reported at min_len 1 without the flood of its other occurrences.
 * pm_hip_set_windows(obj, min_start, max_end, n): after compile() (-1
 * before); -2 for a wrong n, a NULL array or a min_start above 0x7FFFFFFF.
 * A byte string added twice has the window of the add that wins.  The first
 * call allocates one table of 16 bytes per pattern (+ 1 entry) on the device,
 * counted in pm_hip_table_bytes from then on; a later call overwrites it in
 * place after a device synchronize (no window scan may be in flight).
 * compile() and the compiled-image cache do not see windows, and an object
 * that never calls it behaves exactly as before.
 * pm_hip_pattern_window(obj, gid, &min_start, &max_end): 0; -1 for a gid out
 * of range or before pm_hip_set_windows (either pointer may be NULL).
 * pm_hip_scan_batch_windows_device takes the arguments of
 * pm_hip_scan_batch_groups_device; pm_hip_scan_flows_windows_device those of
 * pm_hip_scan_flows_groups_device plus d_pos_in, a DEVICE pointer to nseg
 * uint64_t, 8-byte aligned, the bytes each flow had before this call (NULL =
 * every flow at byte 0), and d_pos_out (NULL = not wanted; -2 if it equals
 * d_pos_in), which receives d_pos_in[j] + offsets[j+1] - offsets[j]; an empty
 * stream copies its position, also in the n == 0 copy pass.  Flow states do
 * not depend on windows, masks or positions: d_state_out is the dense flow
 * call's.  Every other rule is the group siblings'; one new code, -8:
 * pm_hip_set_windows was not called (nothing is launched or written).  The
 * calls allocate nothing and may be captured.
 * The host forms work like pm_hip_read_*_groups; the flow form's pos is a
 * HOST array of nseg uint64_t, read and overwritten like state (NULL = all
 * zero, nothing returned).
 * Measured (64 MiB, all form, every stream on all groups, fresh flows;
 * profiles/windows/): with every window unbounded the calls take, over the
 * group calls of the same run, 1.005-1.023x (batched) and 1.030-1.037x (flow)
 * on random ASCII, 1.042-1.048x and 1.121-1.142x on the lines stream, where
 * every position walks a deep chain and each member costs one more 16-byte
 * table entry; with a third of the patterns limited to the first 256 bytes
 * 0.998-1.023x / 1.026-1.035x on ASCII and 1.032-1.040x / 1.094-1.126x on
 * lines.  At min_len 1 with every pattern of at most 2 bytes anchored at
 * (0, len) a 64 MiB call takes 521-947 us batched and 452-605 us as flows on
 * ASCII (the dense-id call: 485-817 and 362-438 us), 6.7-9.2 ms and 2.8-3.6
 * ms on lines (4.2-5.8 and 1.2-1.3 ms).
 */
int pm_hip_set_windows(void* obj, const uint32_t* min_start, const uint32_t* max_end, size_t n);
int pm_hip_pattern_window(void* obj, uint32_t gid, uint32_t* min_start, uint32_t* max_end);
int pm_hip_scan_batch_windows_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                                     int64_t n, const uint32_t* d_stream_groups, uint32_t min_len, int all,
                                     uint64_t* d_events, uint64_t cap, unsigned long long* d_nevents,
                                     void* hip_stream);
int pm_hip_scan_flows_windows_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                                     int64_t n, const uint32_t* d_state_in, uint32_t* d_state_out,
                                     const uint32_t* d_stream_groups, uint32_t min_len, int all, uint64_t* d_events,
                                     uint64_t cap, unsigned long long* d_nevents, void* hip_stream,
                                     const uint64_t* d_pos_in, uint64_t* d_pos_out);
int pm_hip_read_batch_windows(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg,
                              const uint32_t* stream_groups, uint32_t min_len, int all, uint64_t* events, size_t cap,
                              size_t* nevents);
int pm_hip_read_flows_windows(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg, uint32_t* state,
                              uint64_t* pos, const uint32_t* stream_groups, uint32_t min_len, int all,
                              uint64_t* events, size_t cap, size_t* nevents);

/*
 * Nocase: a per-pattern case-insensitivity flag (Snort's and Suricata's
 * `nocase`), honoured exactly inside the batched and the flow match-list
 * scans, beside the group and window tests.  One automaton is built over the
 * case-FOLDED patterns and walked over case-folded text; a case-sensitive
 * pattern is then confirmed in the kernel against the real bytes.
 * Folding: fold(c) = c + 32 for 'A' <= c <= 'Z', else c -- ASCII only: 0x40,
 * 0x5B, 0x60, 0x7B and bytes >= 0x80 are themselves; a byte "is upper" iff it
 * lies in 'A'..'Z'.
 * Pattern h (bytes p, L of them) ENDS at position i of a stream iff the
 * stream has at least L bytes through i and, for the L bytes t ending at i,
 * fold(t[k]) == fold(p[k]) for all k where nocase[h] != 0, t[k] == p[k] for
 * all k where it is 0.  For a flow the earlier calls' bytes count: a pattern
 * that straddles a packet boundary is found.  h is VISIBLE at i of stream j
 * iff it ends there, has at least min_len bytes, and -- where
 * pm_hip_set_groups was called -- groups[h] & stream_groups[j] != 0, and --
 * where pm_hip_set_windows was called -- it passes its window there (E as in
 * "pattern windows").  Both tables are optional here.
 *   all != 0: one event i << 24 | gid(h) per visible h.
 *   all == 0: at most one event per position, the longest visible pattern;
 *     among visible patterns of equal length the smallest gid.
 * Gids are the object's own, one per byte string as added: "GET" and "get"
 * stay two patterns with two gids and each may be of either kind.  A byte
 * string added twice has the flag of the add that wins.
 * pm_hip_set_nocase(obj, nocase, n): after compile() (-1 before); -2 for a
 * wrong n or NULL.  Builds the images of the folded dictionary for the images
 * the object holds (the reverse trie for rt / auto, the dense rows for ac /
 * auto, both cases' columns holding the same word) with the flattener and
 * the compiled-image cache of compile(), and uploads them with the class
 * tables ("nocase"); all of it counts in pm_hip_table_bytes from
 * then on.  A later call (a rule reload) waits for the device, frees the
 * earlier tables and builds anew.  An object that never calls it behaves,
 * allocates and launches exactly as before.
 * pm_hip_pattern_nocase(obj, gid): 0 / 1; -1 for a gid out of range or
 * before pm_hip_set_nocase.
 * pm_hip_nocase_flow_states: the states of the folded automaton.  The flow
 * form's states are ITS states, a space of their own (0 .. that - 1, 0 =
 * fresh), not interchangeable with pm_hip_scan_flows_device's; the host form
 * checks them against this bound.
 * pm_hip_case_words: W, the u64 words of case history per flow.  A case-
 * sensitive pattern that began in an earlier packet cannot be confirmed from
 * this call's bytes; given the folded match, t[k] == p[k] iff both are upper
 * or neither, so one bit per earlier byte is enough.  W = ceil((Lcs - 1) /
 * 64), Lcs the longest case-sensitive pattern that holds an ASCII letter (0
 * if none: both pointers are then ignored).  d_case_in / d_case_out: DEVICE
 * arrays of nseg * W uint64_t, 8-byte aligned and distinct (-2 if equal);
 * either may be NULL (in: all zero; out: not wanted).  Bit b of word j * W +
 * w is 1 iff the byte 64 w + b + 1 places before stream j's first byte of
 * this call was upper; d_case_out is the same window moved on by the
 * stream's bytes (old bits move up where the packet is shorter than 64 W; an
 * empty packet copies its words, also in the n == 0 copy pass).
 * The scan calls take the arguments of the window siblings plus, for flows,
 * the two histories; return codes, alignment, memory safety, cursor and cap
 * rules, the nseg == 0 / n == 0 cases and capturability (nothing is
 * allocated) are theirs.  One new code, -9: pm_hip_set_nocase was not
 * called.  -7: stream masks without group tables; -6: the object's kind has
 * no folded image for this scan (or the folded dictionary is past the
 * reverse-trie encoding).  d_pos_in / d_pos_out are used only where windows
 * are set.  The flow call launches a second small kernel for d_case_out.
 * The host forms work like pm_hip_read_*_windows; case_hist is a HOST array
 * of nseg * W uint64_t read and overwritten like state and pos (NULL = all
 * zero, nothing returned).
 * pm_hip_nocase_stats: wall ms of the last pm_hip_set_nocase as a whole and
 * of its uploads, and the table bytes it added; -1 before it.
 * Measured (64 MiB, all form, min_len 3, every window unbounded, fresh flows;
 * profiles/nocase/), over the window call of the same run: with every pattern
 * nocase (no confirmation; a list 4.3-4.5x as long on random ASCII) 1.29-1.41x
 * batched and 1.37-1.41x flow on ASCII, 1.14-1.16x and 1.38-1.40x on the lines
 * stream; with no pattern nocase (the window call's list, 0.25-0.33
 * confirmations per byte on lines) 1.40-1.51x and 1.60-1.67x on ASCII,
 * 1.59-1.65x and 4.95-6.00x on lines.  pm_hip_set_nocase takes 0.45-0.89 s
 * and adds 518-737 MB (snort, merged: the folded dense rows).
 */
int pm_hip_set_nocase(void* obj, const uint8_t* nocase, size_t n);
int pm_hip_pattern_nocase(void* obj, uint32_t gid);
uint32_t pm_hip_nocase_flow_states(void* obj);
uint32_t pm_hip_case_words(void* obj);
int pm_hip_nocase_stats(void* obj, double* build_ms, double* upload_ms, size_t* table_bytes);
int pm_hip_scan_batch_nocase_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                                    int64_t n, const uint32_t* d_stream_groups, uint32_t min_len, int all,
                                    uint64_t* d_events, uint64_t cap, unsigned long long* d_nevents,
                                    void* hip_stream);
int pm_hip_scan_flows_nocase_device(void* obj, const uint8_t* d_text, const int64_t* d_offsets, int64_t nseg,
                                    int64_t n, const uint32_t* d_state_in, uint32_t* d_state_out,
                                    const uint32_t* d_stream_groups, uint32_t min_len, int all, uint64_t* d_events,
                                    uint64_t cap, unsigned long long* d_nevents, void* hip_stream,
                                    const uint64_t* d_pos_in, uint64_t* d_pos_out, const uint64_t* d_case_in,
                                    uint64_t* d_case_out);
int pm_hip_read_batch_nocase(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg,
                             const uint32_t* stream_groups, uint32_t min_len, int all, uint64_t* events, size_t cap,
                             size_t* nevents);
int pm_hip_read_flows_nocase(void* obj, const uint8_t* buf, const int64_t* offsets, size_t nseg, uint32_t* state,
                             uint64_t* pos, uint64_t* case_hist, const uint32_t* stream_groups, uint32_t min_len,
                             int all, uint64_t* events, size_t cap, size_t* nevents);

/*
 * Per-stream sets: a match list grouped by stream, on the device.  The ten
 * list scans above leave one unordered array of position << 24 | gid events
 * behind one cursor; a rule engine asks, per packet, flow or line, WHICH
 * patterns hit that stream.  One call turns any such list into per-stream
 * ranges in CSR form and, with PM_BY_STREAM_UNIQUE, keeps one event per
 * (stream, pattern).
 * Input: d_events, cap and d_nevents are exactly what a list scan left
 * behind; the call uses the first min(*d_nevents, cap) events and reads the
 * cursor on the device, so it may be enqueued right behind the scan with no
 * synchronize between.  d_offsets (nseg + 1 values) and nseg are the scan's.
 * An event at position p belongs to the stream j with offsets[j] <= p <
 * offsets[j+1]; empty streams own nothing; an event outside [offsets[0],
 * offsets[nseg]) is dropped.
 * Output: d_stream_ptr gets nseg + 1 values: stream j's events are
 * d_out[ptr[j] .. ptr[j+1]), ptr[0] == 0, ptr[nseg] = the events kept.
 * Events keep their format and their buffer-global position.  flags == 0:
 * the kept events are the used events inside a stream, as a multiset.
 * PM_BY_STREAM_UNIQUE: one event per distinct (stream, gid), carrying the
 * smallest position that gid has in that stream -- a deterministic set.
 * Order inside a stream's range is unspecified on the device; the host form
 * and the twin sort each range ascending.  d_stream_ptr is always complete
 * and exact, whatever out_cap is; an event whose slot is >= out_cap is not
 * stored and nothing at or past d_out[out_cap] is written (out_cap >= cap can
 * never fall short).
 * The call allocates nothing, runs asynchronously on hip_stream with no host
 * synchronize inside (it may be captured), and asks the resident read_block
 * server to leave the device first, like every device launch.  Scratch comes
 * from the caller, 16-byte aligned, pm_hip_by_stream_scratch_bytes(cap, nseg,
 * flags) bytes exactly:
 *     A + r16(8 nseg) + r16(8 ceil(nseg / 1024))
 *     A = r16(4 cap)                              flags == 0 (a stream index per event)
 *     A = 20 T, T = the power of two >= max(2 cap, 64)   PM_BY_STREAM_UNIQUE (the hash
 *                                                 table: a key, a position and a rank per slot)
 * with r16 rounding up to 16 (the streams' counts and the scan's block sums
 * follow A); (size_t)-1 for arguments the call would reject.
 * Returns 0; -1 before compile(); -2 bad arguments, one message for all of:
 * a NULL pointer (d_events with cap > 0, d_out with out_cap > 0, d_nevents,
 * d_offsets, d_stream_ptr, d_scratch) or a misaligned one (8 bytes; d_scratch
 * 16), nseg < 0 or >= 2^31, cap > 2^40, unknown flag bits, d_out == d_events,
 * scratch_bytes too small; -3 launch error.  Nothing is written when a check
 * fails.  nseg == 0: returns 0 and launches nothing.  cap == 0 with nseg > 0:
 * an all-zero d_stream_ptr.
 * Memory safety does not depend on the data: stream indices are clamped into
 * [0, nseg); garbage or unsorted offsets and garbage events give an
 * unspecified grouping, never an access outside the arrays named here.
 * pm_hip_events_by_stream: the host form.  events (nevents of them), offsets
 * and the outputs are HOST arrays; it stages them on the object's batch
 * stream (staging counted in pm_hip_scratch_bytes), runs the device call with
 * room for every event, sorts each stream's range ascending and hands over
 * stream_ptr and the first min(out_cap, kept) events.
 * pm_flat_events_by_stream: the same contract on the host alone -- no
 * handle, no device; -2 as above where it applies (it sets no message).
 * Measured (64 MiB, all-matches lists at min_len 3; profiles/bystream/): the
 * call alone takes, over the scan that made its list, 0.04-0.09x (plain) and
 * 0.09-0.17x (UNIQUE) on random ASCII (51-70 thousand events), 0.08-0.25x and
 * 0.29-1.01x on the lines stream (15-17 million events: 0.32-0.61 ms and
 * 1.3-2.4 ms); over device-to-host copy + sort + searchsorted on the host
 * 0.035-0.25x on ASCII and 0.0015-0.0098x on lines.  UNIQUE keeps 0.999 / 0.94
 * of an ASCII list in 1,500-byte / 100 KiB streams, 0.70 / 0.30 of a lines list.
 */
#define PM_BY_STREAM_UNIQUE 1u
size_t pm_hip_by_stream_scratch_bytes(uint64_t cap, int64_t nseg, uint32_t flags);
int pm_hip_events_by_stream_device(void* obj, const uint64_t* d_events, uint64_t cap,
                                   const unsigned long long* d_nevents, const int64_t* d_offsets, int64_t nseg,
                                   uint32_t flags, uint64_t* d_out, uint64_t out_cap, int64_t* d_stream_ptr,
                                   void* d_scratch, size_t scratch_bytes, void* hip_stream);
int pm_hip_events_by_stream(void* obj, const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                            uint32_t flags, uint64_t* out, size_t out_cap, int64_t* stream_ptr);
int pm_flat_events_by_stream(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                             uint32_t flags, uint64_t* out, size_t out_cap, int64_t* stream_ptr);

/*
 * Rules: which multi-pattern rules fire in each stream, on the device.  A
 * rule engine's rule is several patterns, some of them negated (Snort's
 * content: and content:!, Hyperscan's logical combinations).  One call takes
 * the list a scan left behind and gives, per stream, the rules that fired.
 * A rule is a list of 1 to 64 terms; a term is a pattern gid (the number the
 * events carry in their low 24 bits), positive or negated.  Over one stream
 * let S be the set of gids with at least one used event inside the stream.
 * The rule fires in the stream iff every positive term's gid is in S and no
 * negated term's gid is.  The position of the hit is the largest of the first
 * (smallest) positions its positive terms have in the stream: the byte at
 * which the conjunction became true; negations do not move it.  Positions are
 * buffer-global, as in the events.  A hit is position << 24 | rule, rule the
 * rule's 0-based index: the events' own format.  The hits are a pure function
 * of the used events, the offsets and the rules: duplicate events, events
 * outside every stream, the order of the list and the choice of anchors
 * change nothing.
 * Rules see only what the list holds.  For exact rule semantics scan
 *   - with an all-matches form (all != 0; pm_hip_scan_*_matches_device is
 *     one): the longest-match forms drop the patterns that end at a position
 *     beside a longer one;
 *   - at a min_len no larger than the shortest term (pm_hip_rules_min_len):
 *     a scan leaves out every pattern shorter than its min_len;
 *   - with a cap that holds the whole list: an overflowed list lacks events,
 *     so positive terms may miss and negated ones pass.
 * This call knows no flows: a rule is evaluated over the streams of one call,
 * and no set is carried from one packet of a flow to the next.  The flow rules
 * below (pm_hip_flow_rules_device) carry a set per flow.
 * pm_hip_set_rules: the rules in CSR form.  term_ptr has nrules + 1 values,
 * starts at 0 and does not decrease; rule r's terms are terms[term_ptr[r] ..
 * term_ptr[r+1]).  A term holds the gid in bits 0-23; PM_RULE_NEGATED (bit
 * 31) marks a negated term; PM_RULE_FAST (bit 30) marks the rule's anchor,
 * the caller's fast_pattern: the term at whose (stream, gid) the rule is
 * verified.  Without one the anchor is the positive term with the longest
 * pattern, ties going to the smaller gid.  After compile() only: -1 before.
 * -2, with one message naming every constraint, for: a NULL array; nrules 0
 * or above 2^24; a rule with 0 or more than 64 terms; a rule with no positive
 * term; a gid that names no pattern (pm_hip_pattern_len(obj, gid) == 0); a gid
 * twice in one rule; bits besides the three fields; two PM_RULE_FAST terms in
 * one rule or one on a negated term.  Nothing changes on an error.  The call
 * builds the device tables (an inverted index gid -> the rules anchored at
 * it, and each rule's other terms, positive ones first), counted in
 * pm_hip_table_bytes.  A later call replaces them after a device synchronize,
 * like pm_hip_set_windows: no rules call may be in flight.  compile() and the
 * compiled-image cache do not see rules, and an object that never calls this
 * behaves exactly as before.
 * pm_hip_rule_count: the rules set (0 before).  pm_hip_rules_min_len: the
 * length of the shortest pattern any term names (0 before pm_hip_set_rules).
 * pm_hip_rules_by_stream_device: d_events, cap, d_nevents, d_offsets and nseg
 * are exactly those of pm_hip_events_by_stream_device: the raw list behind
 * its device cursor, of which min(*d_nevents, cap) events are used, the
 * cursor read on the device, so the call may be enqueued right behind the
 * scan with no synchronize between.  Output: d_rule_ptr gets nseg + 1 int64
 * values; stream j's hits are d_hits[ptr[j] .. ptr[j+1]), in unspecified
 * order inside a range; ptr[0] == 0, ptr[nseg] = the hits.  d_rule_ptr is
 * complete and exact whatever hits_cap is; a hit whose slot is >= hits_cap is
 * not stored and nothing at or past d_hits[hits_cap] is written.  The number
 * of hits is NOT bounded by cap (one event can anchor many rules), so the
 * exact d_rule_ptr[nseg] is what a caller sizes a retry from.  The call
 * allocates nothing, runs asynchronously on hip_stream with no host
 * synchronize inside (it may be captured), and asks the resident read_block
 * server to leave the device first, like every device launch.  Scratch comes
 * from the caller, 16-byte aligned, pm_hip_rules_scratch_bytes(cap, nseg)
 * bytes exactly:
 *     16 T + r16(8 nseg) + r16(8 ceil(nseg / 1024))
 * T = the power of two >= max(2 cap, 64), the by-stream call's table (a key
 * and a position per slot), r16 rounding up to 16 (the streams' counts and
 * the scan's block sums follow the table); (size_t)-1 for arguments the call
 * would reject.
 * Returns 0; -1 before compile(); -2 bad arguments, one message for all of:
 * a NULL pointer (d_events with cap > 0, d_hits with hits_cap > 0, d_nevents,
 * d_offsets, d_rule_ptr, d_scratch) or a misaligned one (8 bytes; d_scratch
 * 16), nseg < 0 or >= 2^31, cap > 2^40, d_hits == d_events, scratch_bytes too
 * small; -10 pm_hip_set_rules was not called; -3 launch error.  Nothing is
 * launched or written when a check fails.  nseg == 0: returns 0 and launches
 * nothing.  cap == 0 with nseg > 0: an all-zero d_rule_ptr.
 * Memory safety does not depend on the data: stream indices are clamped into
 * [0, nseg), a gid above the last pattern anchors nothing, probe indices are
 * masked by the table size; garbage offsets or events give unspecified hits,
 * never an access outside the arrays named here.
 * pm_hip_rules_by_stream: the host form.  events (nevents of them), offsets
 * and the outputs are HOST arrays; it stages them on the object's batch
 * stream (staging counted in pm_hip_scratch_bytes), runs the device call (a
 * second time where its hits array was too short), sorts each stream's range
 * ascending and hands over rule_ptr and the first min(hits_cap, total) hits.
 * -1, -2 (a NULL array, nseg >= 2^31, nevents > 2^40, hits == events), -10 and
 * -3 as above.
 * pm_flat_rule_tables, pm_flat_rules_by_stream: the host alone, no handle and
 * no device; they set no message.  pm_flat_rule_tables runs every check of
 * pm_hip_set_rules (pattern_len: npat + 1 lengths by gid, [0] == 0; a gid
 * above npat names no pattern), picks each rule's anchor and returns the
 * inverted index in CSR form: anchor_ptr_out[npat + 2] by gid,
 * anchor_rules_out[nrules] the rules anchored at each gid, ascending inside a
 * gid's range, anchor_term_out[nrules] the index in terms of each rule's
 * anchor; 0, or -2 with nothing written.  pm_flat_rules_by_stream is the twin
 * of the device call over host arrays, each range sorted ascending; it needs
 * no anchors and no dictionary (it checks everything about the rules but
 * whether a gid names a pattern); 0, or -2.
 * Measured (64 MiB, all-matches lists at min_len 3, 10,000 synthetic rules of
 * 2-4 positive terms, a fifth with a negated one; profiles/rules/): the call
 * alone takes 0.045-0.053 ms on random ASCII (51-70 thousand events) and
 * 1.9-2.6 ms on the lines stream (15-17 million events): 0.07-0.16x and
 * 0.40-1.14x the scan that made its list (above it only behind the flow scan
 * on lines), 0.68-1.57x the PM_BY_STREAM_UNIQUE call on the same list, and
 * 0.0028-0.0137x the UNIQUE sets copied to the host and walked by
 * pm_flat_rules_by_stream on one thread.  5,000 rules more on one frequent
 * anchor: 0.5-0.7 ms on ASCII, 2.3-12 ms on lines ("Rules").
 */
#define PM_RULE_NEGATED 0x80000000u
#define PM_RULE_FAST 0x40000000u
int pm_hip_set_rules(void* obj, const uint32_t* term_ptr, const uint32_t* terms, size_t nrules);
size_t pm_hip_rule_count(void* obj);
uint32_t pm_hip_rules_min_len(void* obj);
size_t pm_hip_rules_scratch_bytes(uint64_t cap, int64_t nseg);
int pm_hip_rules_by_stream_device(void* obj, const uint64_t* d_events, uint64_t cap,
                                  const unsigned long long* d_nevents, const int64_t* d_offsets, int64_t nseg,
                                  uint64_t* d_hits, uint64_t hits_cap, int64_t* d_rule_ptr, void* d_scratch,
                                  size_t scratch_bytes, void* hip_stream);
int pm_hip_rules_by_stream(void* obj, const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                           uint64_t* hits, size_t hits_cap, int64_t* rule_ptr);
int pm_flat_rule_tables(const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, const uint32_t* pattern_len,
                        size_t npat, uint32_t* anchor_ptr_out, uint32_t* anchor_rules_out, uint32_t* anchor_term_out);
int pm_flat_rules_by_stream(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                            const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, uint64_t* hits,
                            size_t hits_cap, int64_t* rule_ptr);

/*
 * Flow rules: rules whose terms lie in different packets of one flow.  The
 * flow scans (pm_hip_scan_flows_*_device) are exact across packet cuts: they
 * report a pattern that begins in one call and ends in the next.  The flow
 * rules are the rules behind them: the caller keeps one set of term bits per
 * live flow ON THE DEVICE, and one call, behind any list scan, reports the
 * rules whose conjunction became true in this call's bytes and folds this
 * call's patterns into the flows' sets.
 * Rule set.  pm_hip_set_flow_rules takes a rule set of its own, in the CSR
 * form, with the term format and every check of pm_hip_set_rules (1 to 64
 * terms, PM_RULE_NEGATED, PM_RULE_FAST; -1 before compile(); -2, with one
 * message naming every constraint, for the same cases; nothing changes on an
 * error).  It is independent of pm_hip_set_rules, which it does not touch: an
 * object may hold both sets, neither, or either one.  Its device tables (the
 * bit of each gid; an inverted index from EVERY positive term's gid to the
 * rules that carry it; each rule's full term list, the PM_RULE_FAST term --
 * else the longest positive pattern, ties to the smaller gid -- first, then
 * the other positive terms, then the negated ones) live in allocations of
 * their own, counted in pm_hip_table_bytes, replaced by a later call after a
 * device synchronize (no flow-rules call may be in flight) and freed with the
 * object; compile() and the compiled-image cache do not see them.
 * PM_RULE_FAST cannot gate verification here, because the anchor may be a
 * carried term: it is accepted and only decides which term is tested first.
 * pm_hip_flow_rule_count: the rules set (0 before).
 * pm_hip_flow_rules_min_len: the length of the shortest pattern any term
 * names (0 before).
 * Bits.  K is the number of distinct gids named by any term, positive or
 * negated.  The bit of a gid is its rank among those gids, ascending.  A
 * flow's set has W = max(1, ceil(K / 64)) u64 words (pm_hip_flow_rule_words;
 * 0 before); bit b lives in word b >> 6 at bit b & 63.  Bits at or above K
 * are ignored when read and never set.  The numbering is public --
 * pm_hip_flow_rule_bit(obj, gid): the bit, or -1 for a gid that no term names
 * and before pm_hip_set_flow_rules; pm_flat_flow_rule_bits on the host alone
 * -- so the host twin's sets and the device's are bit-identical.
 * State.  d_sets is a device array of nrows x W u64, owned by the caller, a
 * row per live flow.  d_rows[j] (int64, nseg of them) names the row of the
 * call's stream j; NULL means stream j uses row j, which needs nrows >= nseg.
 * A zeroed row is a fresh flow, and the caller ends a flow by zeroing its
 * row.  A row index outside [0, nrows) makes its stream inert: no hits,
 * nothing written.  One row named by two streams of one call gives
 * unspecified sets and hits for those streams, never an access outside the
 * arrays.
 * Semantics: the rules semantics above, applied to the flow's prefix.  Let C
 * be the gids whose bit is set in the flow's row before the call (the carried
 * terms), and N the term gids with at least one used event inside the stream
 * in this call that are not in C, each with its first (smallest) position in
 * this call.  Rule r gives a hit in this call iff every positive term is in
 * C u N, at least one positive term is in N, and no negated term is in C u N.
 * The hit is position << 24 | r with the largest first position among the
 * positive terms in N: buffer-global, the events' own format (carried terms
 * became true in earlier calls and cannot be the largest).  This equals the
 * hits of pm_hip_rules_by_stream_device over everything the flow has had
 * through this call, scanned as one stream, restricted to the hits whose
 * position lies in this call's bytes.  So:
 *   - a rule fires at most once per flow;
 *   - a negated term seen in an earlier call, or anywhere in this call (even
 *     after the completing byte), suppresses the rule;
 *   - a negated term that first appears in a later call does not retract a
 *     hit already reported.
 * Commit.  After the hits are written, every gid of N has its bit OR-ed into
 * its flow's row.  With PM_FLOW_RULES_KEEP in flags the rows are left
 * untouched: a count-only or dry call, used to size hits_cap.  Without it
 * the rows are updated whatever hits_cap is, and d_rule_ptr is exact either
 * way, as in the rules call.  After a commit the same call reports nothing
 * (every term is carried), so a caller who cannot bound the hits sizes them
 * with a PM_FLOW_RULES_KEEP call first and then commits once.
 * The list has the rules call's preconditions: an all-matches form, at a
 * min_len <= pm_hip_flow_rules_min_len, with a cap that held the list; and it
 * must come from a flow scan that continued the same flows, which is what
 * makes a pattern that straddles a cut appear.  Otherwise the call does not
 * care which scan made the list: plain, group, window and nocase lists work.
 * pm_hip_flow_rules_device: d_events, cap, d_nevents, d_offsets, nseg,
 * d_hits, hits_cap, d_rule_ptr, d_scratch, scratch_bytes and hip_stream are
 * exactly those of pm_hip_rules_by_stream_device, with its guarantees: the
 * cursor is read on the device; the call allocates nothing, does not
 * synchronize on the host and may be captured; it asks the resident
 * read_block server to leave the device first; hits inside a range come in
 * unspecified order and nothing at or past d_hits[hits_cap] is written.
 * Scratch: pm_hip_flow_rules_scratch_bytes(cap, nseg) bytes exactly, the
 * rules call's formula:
 *     16 T + r16(8 nseg) + r16(8 ceil(nseg / 1024))
 * T = the power of two >= max(2 cap, 64), r16 rounding up to 16; (size_t)-1
 * for arguments the call would reject.
 * Returns 0; -1 before compile(); -2 bad arguments, one message for all of
 * the rules call's cases and: d_sets NULL with nrows > 0, d_sets or d_rows
 * misaligned (8 bytes), nrows < 0 or nrows x W above 2^40 words, d_rows NULL
 * with nrows < nseg, a flag bit other than PM_FLOW_RULES_KEEP; -11
 * pm_hip_set_flow_rules was not called (whether or not pm_hip_set_rules was);
 * -3 launch error.  Nothing is launched or written when a check fails.
 * nseg == 0: returns 0 and launches nothing.  cap == 0 with nseg > 0: an
 * all-zero d_rule_ptr and untouched sets.
 * Memory safety does not depend on the data: beyond the rules call's clamps a
 * row index is tested against nrows wherever it is read, a bit against 64 W
 * and an index range against the index array; garbage offsets, events, rows
 * or sets give unspecified hits and sets, never an access outside the arrays
 * named here.
 * pm_hip_flow_rules: the host form.  events, offsets, sets (nrows x W,
 * updated in place), rows (nseg of them, or NULL) and the outputs are HOST
 * arrays; it stages them on the object's batch stream (staging counted in
 * pm_hip_scratch_bytes) and runs the device call so that the committing call
 * runs exactly once: where its hits staging may be too short it counts the
 * hits with a PM_FLOW_RULES_KEEP call first.  It sorts each stream's range
 * ascending, hands over rule_ptr and the first min(hits_cap, total) hits and
 * copies the sets back.  -1, -2, -11 and -3 as above where they apply.
 * pm_flat_flow_rule_bits, pm_flat_flow_rules: the host alone, no handle and
 * no device; they set no message.  pm_flat_flow_rule_bits runs the checks of
 * pm_hip_set_flow_rules that need no pattern lengths (a gid must lie in [1,
 * npat]) and gives bit_by_gid_out[npat + 1] (0xFFFFFFFF: no term) and
 * *nbits_out = K; 0, or -2 with nothing written.  pm_flat_flow_rules is the
 * twin of the device call over host arrays, the sets updated in place, each
 * range sorted ascending; words must be the rule set's W; 0, or -2 for what
 * the device call rejects (and a wrong words), with nothing written.
 * Measured (snort, 64 MiB in 44,740 packets of 1,500 bytes, one per flow and
 * call, two calls behind the flow scan at min_len 3, 10,000 synthetic rules
 * over 20,981 term gids, W = 328; profiles/flowrules/): the call alone takes
 * 0.12 ms on random ASCII (51 thousand events), 0.32x the scan, and 8.9-10.2
 * ms on the lines stream (14.6 million events), 3.7-4.4x the scan; against
 * the UNIQUE sets copied to the host and walked by pm_flat_flow_rules on one
 * thread 0.0060-0.0079x ("Flow rules").
 */
#define PM_FLOW_RULES_KEEP 1u
int pm_hip_set_flow_rules(void* obj, const uint32_t* term_ptr, const uint32_t* terms, size_t nrules);
size_t pm_hip_flow_rule_count(void* obj);
uint32_t pm_hip_flow_rules_min_len(void* obj);
uint32_t pm_hip_flow_rule_words(void* obj);
int64_t pm_hip_flow_rule_bit(void* obj, uint32_t gid);
size_t pm_hip_flow_rules_scratch_bytes(uint64_t cap, int64_t nseg);
int pm_hip_flow_rules_device(void* obj, const uint64_t* d_events, uint64_t cap, const unsigned long long* d_nevents,
                             const int64_t* d_offsets, int64_t nseg, uint64_t* d_sets, int64_t nrows,
                             const int64_t* d_rows, uint32_t flags, uint64_t* d_hits, uint64_t hits_cap,
                             int64_t* d_rule_ptr, void* d_scratch, size_t scratch_bytes, void* hip_stream);
int pm_hip_flow_rules(void* obj, const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                      uint64_t* sets, size_t nrows, const int64_t* rows, uint32_t flags, uint64_t* hits,
                      size_t hits_cap, int64_t* rule_ptr);
int pm_flat_flow_rule_bits(const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, size_t npat,
                           uint32_t* bit_by_gid_out, uint32_t* nbits_out);
int pm_flat_flow_rules(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                       const uint32_t* term_ptr, const uint32_t* terms, size_t nrules, uint64_t* sets, size_t nrows,
                       size_t words, const int64_t* rows, uint32_t flags, uint64_t* hits, size_t hits_cap,
                       int64_t* rule_ptr);

/*
 * Ordered rules: rules whose terms must follow one another, at a distance
 * (Snort's relative content: content:"A"; content:"B"; distance:N;).  The
 * rules above are unordered sets; here a positive term may have to begin at
 * least d bytes after the term before it has ended.
 * An event position << 24 | gid says that pattern gid, of L(gid) bytes, ends
 * at buffer byte position: the occurrence covers [position - L + 1, position].
 * An ordered rule is a rule of pm_hip_set_rules (1 to 64 terms; bits 0-23 the
 * gid, PM_RULE_NEGATED, PM_RULE_FAST) and a parallel uint32_t gaps[], one
 * value per term:
 *   - PM_SEQ_FREE (0xFFFFFFFF): the term is as in the rules above: it may lie
 *     anywhere in the stream;
 *   - d in [0, 0x7FFFFFFF]: the term FOLLOWS the nearest positive term listed
 *     before it in the rule (negated terms in between are skipped).  For a
 *     term t that follows u, the occurrence chosen for t must begin at least d
 *     bytes after the one chosen for u has ended: p_t - L_t + 1 >= p_u + 1 + d,
 *     that is p_t >= p_u + d + L_t.  d = 0 is Snort's distance:0.
 * Terms linked this way form chains; a free positive term starts a chain,
 * possibly of length 1.
 * Firing.  The rule fires in a stream iff some choice of one occurrence inside
 * the stream per positive term satisfies every link, and no negated term's
 * gid has an occurrence in the stream.  The position of the hit is the
 * smallest, over all valid choices, of the largest chosen position: the byte
 * at which the stream's prefix first satisfies the positive part; negations
 * do not move it.  A hit is position << 24 | rule as above; the output is the
 * rules call's CSR form (d_rule_ptr[nseg + 1], exact whatever hits_cap is), a
 * pure function of the used events, the offsets and the rules.  With every
 * gap PM_SEQ_FREE the hits are those of pm_hip_rules_by_stream_device.  The
 * call chooses greedily -- a chain's head at its first position, each follower
 * at its first position that satisfies the link -- which is exact because
 * positions grow along a chain and an earlier choice never rules out a later
 * one (the proof is in DESIGN.md §4, "Ordered rules").
 * The list has the rules call's preconditions: an all-matches form, at a
 * min_len <= pm_hip_seq_rules_min_len, with a cap that held the list.
 * Out of scope: negative distances and relative negated terms.  This call
 * knows no flows; the flow ordered rules below (pm_hip_flow_seq_rules_device)
 * carry each chain's progress from one packet of a flow to the next.
 * Within: an upper bound on a link.  Beside gaps[] a rule set may carry a
 * second parallel uint32_t withins[], one value per term:
 *   - PM_SEQ_FREE: no upper bound; the term is as above;
 *   - w in [0, 0x7FFFFFFF], on a term t that follows u: the occurrence chosen
 *     for t must end at most w bytes after the one chosen for u has ended:
 *     p_t <= p_u + w, beside the lower bound p_t >= p_u + d + L_t.
 * With d == 0 this is Snort's and Suricata's within:w.  w counts from the end
 * of u whatever the distance, as Suricata counts it; a front end that counts
 * within from behind the distance passes d + W.  w == d + L_t places t exactly
 * d bytes behind u.  A within is accepted only on a following term (one whose
 * gap is not PM_SEQ_FREE, so never on a negated term); it is rejected where w
 * < d + L_t, because no occurrence can meet that link (Suricata rejects it
 * too), and in [0x80000000, 0xFFFFFFFE].  Firing and the hit's position are
 * as above, "every link" meaning both bounds.  With an upper bound an earlier
 * choice can rule out a later one and the greedy choice is no longer exact:
 * a set with at least one bound is evaluated by a walk of its own, which is
 * exact (level by level, F_0 = occ(t_0) and F_i = {p in occ(t_i): some f in
 * F_(i-1) has f + d_i + L_i <= p <= f + w_i}; a chain's value is min F_last,
 * the hit the largest over the chains; the walk and its proof are in DESIGN.md
 * §4, "The walk with an upper bound").  A set without any bound runs the
 * greedy kernel as before, and with every within free the hits are the same,
 * hit for hit.
 * pm_hip_set_seq_rules_within(obj, term_ptr, terms, gaps, withins, nrules):
 * pm_hip_set_seq_rules with the bounds; withins == NULL means every value is
 * PM_SEQ_FREE, and pm_hip_set_seq_rules is this call with NULL.  It sets the
 * object's one ordered rule set.  The same return codes, the same message
 * (which names within), the same device synchronize before replacing and the
 * same accounting in pm_hip_table_bytes; the bounds are one more device array
 * of a word per term, by record, uploaded only where the set has a bound.
 * pm_hip_seq_rules_within_run(obj): the longest run of consecutive bounded
 * links in any rule of the set; 0 where there is no bound and before a set.
 * The walk keeps one u32 cursor per level of a run in LDS, 256 x 4 x run
 * bytes per workgroup (at most 63 KiB).  pm_hip_seq_rules_by_stream_device,
 * pm_hip_seq_rules_by_stream and pm_hip_seq_rules_scratch_bytes keep their
 * signatures, return codes, scratch formula and guarantees, and honour the
 * set's bounds.  The walk's loops are bounded by the list's capacity and its
 * reads by the clamped ranges, as the rest of the call's.
 * Measured (profiles/within/; DESIGN.md §4, "The walk with an upper bound"): a
 * set with every later term bounded costs 1.08-1.14x the distance-only set on
 * random ASCII and 1.22-1.27x on the lines stream (the eval pass alone 2x); an
 * unbounded set runs in the parent's time.  The worst case is one lane walking
 * two long ranges whose candidates all fail: 98.6 ms for two ranges of 25,592
 * positions in one 100 KiB stream.
 * pm_hip_set_seq_rules(obj, term_ptr, terms, gaps, nrules): term_ptr and terms
 * as pm_hip_set_rules takes them, gaps parallel to terms.  After compile()
 * only: -1 before.  It runs every check of pm_hip_set_rules, with these
 * differences and additions (-2 with one message naming every constraint;
 * nothing changes on an error): a NULL gaps; a gap on a negated term; a gap on
 * a rule's first positive term; a gap in [0x80000000, 0xFFFFFFFE]; a gid may
 * occur more than once among a rule's positive terms, every occurrence after
 * the first being a following term (A ... A); a gid in two free positive
 * terms and a gid both positive and negated are rejected.  The anchor is
 * chosen as in pm_hip_set_rules: the PM_RULE_FAST term, else the positive term
 * with the longest pattern, ties going to the smaller gid.  The rule set is
 * the object's own: pm_hip_set_rules and pm_hip_set_flow_rules do not see it
 * and are not touched.  Its device tables (the inverted index gid -> the rules
 * anchored at it, and per rule a record {gid | flags, gap, L} per term, the
 * positive ones in listed order, then the negated ones) are counted in
 * pm_hip_table_bytes and replaced by a later call after a device synchronize:
 * no ordered-rules call may be in flight.
 * pm_hip_seq_rule_count: the rules set (0 before).  pm_hip_seq_rules_min_len:
 * the length of the shortest pattern any term names (0 before).
 * pm_hip_seq_rules_by_stream_device: the arguments, the output and the
 * guarantees of pm_hip_rules_by_stream_device: it allocates nothing, runs
 * asynchronously on hip_stream with no host synchronize inside (it may be
 * captured; the list's cursor and the work list's length are read on the
 * device, and the work list's cursor is reset inside the call), and asks the
 * resident read_block server to leave the device first.  Scratch comes from
 * the caller, 16-byte aligned, pm_hip_seq_rules_scratch_bytes(cap, nseg) bytes
 * exactly:
 *     24 T + r16(8 (T + 1)) + r16(8 cap) + r16(4 (cap / 17 + 1)) + 16
 *       + r16(8 ceil(T / 1024)) + r16(8 nseg) + r16(8 ceil(nseg / 1024))
 * T = the power of two >= max(2 cap, 64): the table (a key, a smallest
 * position and a count per slot), the slots' ranges, every used event's
 * position grouped by slot and sorted inside a slot, the work list of the
 * slots with more than 16 positions and its cursor, the block sums of the
 * scan over the slots, the streams' counts and the block sums of the scan
 * over them; (size_t)-1 for arguments the call would reject.
 * Returns 0; -1 before compile(); -2 bad arguments, the rules call's cases; -10
 * pm_hip_set_seq_rules was not called (whether or not pm_hip_set_rules was);
 * -3 launch error.  Nothing is launched or written when a check fails.  nseg
 * == 0: returns 0 and launches nothing.  cap == 0 with nseg > 0: an all-zero
 * d_rule_ptr.
 * Memory safety does not depend on the data: beyond the rules call's clamps a
 * slot's range is clamped into [0, cap] and to begin <= end, a position is
 * stored below cap only, a work-list entry is tested against T, and a
 * bisection stays inside its clamped range; garbage offsets or events give
 * unspecified hits, never an access outside the arrays named here.
 * Sorting.  A slot's range of at most 16 positions is sorted by one lane; a
 * longer one by one workgroup with a bitonic network, in LDS up to 4,096
 * positions, beyond that in parts of 4,096 in LDS and merges whose wide steps
 * run in global memory: O(m log^2 m) for m positions.  The worst case is one
 * pattern ending at every byte of one long stream: all of the list in one
 * range, sorted by one workgroup: 116 ms for 2^20 positions, where the same
 * events in ranges of 16 to 4,096 take 0.5-1.1 ms.
 * Measured (the rules call's cells, lists and 10,000 rules, snort;
 * profiles/seqrules/): 0.084-0.097 ms on random ASCII and 6.9-7.3 ms on the
 * lines stream, 1.8-1.9x and 2.7-3.7x the rules call on the same list (its
 * own spread: 1.000-1.088), the same with every gap free and with every later
 * term at distance 0: the price is the index, not the links (DESIGN.md §4,
 * "Ordered rules").
 * pm_hip_seq_rules_by_stream: the host form, as pm_hip_rules_by_stream: host
 * arrays staged on the object's batch stream, the device call (a second time
 * where its hits array was too short), each stream's range sorted ascending.
 * pm_flat_seq_rule_tables, pm_flat_seq_rules_by_stream: the host alone, no
 * handle and no device; they set no message.  pm_flat_seq_rule_tables runs
 * every check of pm_hip_set_seq_rules (pattern_len: npat + 1 lengths by gid,
 * [0] == 0) and returns pm_flat_rule_tables' outputs; 0, or -2 with nothing
 * written.  pm_flat_seq_rules_by_stream is the twin of the device call over
 * host arrays, each range sorted ascending: greedy over the sorted
 * occurrences of every (stream, gid), with an index of its own and no
 * anchors; it needs pattern_len for the links and runs the same checks; 0, or
 * -2 with nothing written.  pm_flat_seq_rule_tables_within and
 * pm_flat_seq_rules_by_stream_within take withins (NULL: every one free) and
 * run every check of pm_hip_set_seq_rules_within; the twin does not use the
 * device's walk: it computes the feasible sets level by level over each
 * stream's sorted occurrences, per occurrence two bisections in the level
 * before and a prefix count of that level's feasible flags: O(n log n), no
 * backtracking.
 */
#define PM_SEQ_FREE 0xFFFFFFFFu
int pm_hip_set_seq_rules(void* obj, const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                         size_t nrules);
int pm_hip_set_seq_rules_within(void* obj, const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                                const uint32_t* withins, size_t nrules);
uint32_t pm_hip_seq_rules_within_run(void* obj);
int pm_flat_seq_rule_tables_within(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                                   const uint32_t* withins, size_t nrules, const uint32_t* pattern_len, size_t npat,
                                   uint32_t* anchor_ptr_out, uint32_t* anchor_rules_out, uint32_t* anchor_term_out);
int pm_flat_seq_rules_by_stream_within(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                                       const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                                       const uint32_t* withins, size_t nrules, const uint32_t* pattern_len,
                                       size_t npat, uint64_t* hits, size_t hits_cap, int64_t* rule_ptr);
size_t pm_hip_seq_rule_count(void* obj);
uint32_t pm_hip_seq_rules_min_len(void* obj);
size_t pm_hip_seq_rules_scratch_bytes(uint64_t cap, int64_t nseg);
int pm_hip_seq_rules_by_stream_device(void* obj, const uint64_t* d_events, uint64_t cap,
                                      const unsigned long long* d_nevents, const int64_t* d_offsets, int64_t nseg,
                                      uint64_t* d_hits, uint64_t hits_cap, int64_t* d_rule_ptr, void* d_scratch,
                                      size_t scratch_bytes, void* hip_stream);
int pm_hip_seq_rules_by_stream(void* obj, const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                               uint64_t* hits, size_t hits_cap, int64_t* rule_ptr);
int pm_flat_seq_rule_tables(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps, size_t nrules,
                            const uint32_t* pattern_len, size_t npat, uint32_t* anchor_ptr_out,
                            uint32_t* anchor_rules_out, uint32_t* anchor_term_out);
int pm_flat_seq_rules_by_stream(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                                const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps, size_t nrules,
                                const uint32_t* pattern_len, size_t npat, uint64_t* hits, size_t hits_cap,
                                int64_t* rule_ptr);

/*
 * Flow ordered rules: ordered rules (distance only) whose terms lie in
 * different packets of one flow -- content:"A"; content:"B"; distance:N; with
 * A and B in different TCP segments.  The caller keeps one progress row per
 * live flow ON THE DEVICE, and one call, behind any flow list scan, reports
 * the ordered rules that became true in this call's bytes and advances the
 * rows.
 * Rule set.  pm_hip_set_flow_seq_rules(obj, term_ptr, terms, gaps, nrules)
 * takes a rule set of its own, independent of pm_hip_set_rules,
 * pm_hip_set_flow_rules and pm_hip_set_seq_rules: an object may hold any of
 * the four.  It runs every check of pm_hip_set_seq_rules with the same return
 * codes (-1 before compile(); -2 with one message; nothing changes on an
 * error).  withins are not accepted: a bound across packets needs a carried
 * feasible set per level and is out of scope, as are negative distances and
 * relative negated terms.  PM_RULE_FAST is accepted and has no effect on the
 * results.  The device tables (the bit of each gid; an inverted index from
 * every DISTINCT positive gid of a rule to the rule; the ordered rules'
 * records; each rule's first chain word) live in allocations of their own,
 * counted in pm_hip_table_bytes, replaced by a later call after a device
 * synchronize and freed with the object.
 * pm_hip_flow_seq_rule_count: the rules set (0 before).
 * pm_hip_flow_seq_rules_min_len: the shortest pattern any term names (0 before).
 * Row layout.  A row has S = max(1, C + W) u64 words (pm_hip_flow_seq_rule_words;
 * 0 before).
 *   Chain words.  The chains with at least two positive terms are numbered c =
 *   0 .. C - 1, by rule and then by the head's place in the rule
 *   (pm_hip_flow_seq_chain_count = C).  Word c is 0 while the chain's head has
 *   not been seen in the flow; else (E + 1) << 6 | k, where k in 0..63 is the
 *   deepest level chosen so far (0: the head) and E the flow byte index at
 *   which that level's chosen occurrence ends.  A chain is done when k is its
 *   last level.  pm_hip_flow_seq_chain_word(obj, rule, term_index): the word
 *   of the chain headed by that term of that rule, as the rule was given, or -1.
 *   Bits.  K is the number of distinct gids named by a chain of one term or by
 *   a negated term; a gid's bit is its rank among them, ascending
 *   (pm_hip_flow_seq_rule_bit(obj, gid), or -1).  Bit b lives in word C + b /
 *   64 at bit b % 64 and says that the gid has occurred in the flow.  W =
 *   ceil(K / 64).
 * A zeroed row is a fresh flow.  pm_flat_flow_seq_rule_layout gives the same
 * layout on the host alone (chain_word_out: one value per term, 0xFFFFFFFF
 * where the term heads no such chain; bit_by_gid_out[npat + 1], 0xFFFFFFFF: no
 * bit; C, K and S), so the host twin's rows and the device's are bit-identical.
 * Semantics.  For one flow let P_k be the flow's bytes through call k, taken
 * as one stream, its events re-based to flow positions.  The hits of call k
 * are exactly the hits of pm_hip_seq_rules_by_stream_device (distance only)
 * over P_k whose position lies in call k's bytes, reported as position << 24 |
 * rule with the position buffer-global, in the events' own format.  So:
 *   - a rule fires at most once per flow;
 *   - a negated term seen in an earlier call, or anywhere in this call (even
 *     after the completing byte), suppresses the rule;
 *   - a negated term that first appears in a later call retracts nothing.  So
 *     the union of a flow's hits over its calls equals the ordered-rules call's
 *     hits over the uncut flow for every rule without a negated term, whatever
 *     the cuts; for a rule with one, the uncut flow's hits are a subset of the
 *     union: a cut may report a rule that a negation further on would have
 *     suppressed in the flow as a whole;
 *   - a link is measured in flow bytes: a follower in packet 3 may follow a
 *     head in packet 1, and an occurrence that straddles a cut counts with its
 *     true start (a follower that begins before its head has ended does not
 *     satisfy the link, wherever the cut lies).
 * Greedy stays exact across calls: a level's chosen position depends only on
 * the occurrences at or below it and later calls only add larger positions, so
 * a level once chosen never changes ("Flow ordered rules").  A
 * rule fires in a call iff every chain is done, at least one of them reached
 * its last level in this call, and no negated gid is carried or held; the
 * hit's position is the largest completing position of this call.
 * pm_hip_flow_seq_rules_device(obj, d_events, cap, d_nevents, d_offsets, nseg,
 * d_prog, nrows, d_rows, d_pos_in, flags, d_hits, hits_cap, d_rule_ptr,
 * d_scratch, scratch_bytes, hip_stream): the list, the hits, d_rule_ptr,
 * d_rows, nrows, the inert rows and PM_FLOW_RULES_KEEP are exactly those of
 * pm_hip_flow_rules_device, with d_prog (nrows x S u64) in the place of d_sets.
 * d_pos_in is nseg u64, the bytes each flow had before this call, as the
 * window scan takes them; it is required.  A stream with pos_in + length above
 * 2^57 is inert.  Without PM_FLOW_RULES_KEEP the rows are advanced whatever
 * hits_cap is: every chain of a rule with a positive term in this call's bytes
 * is advanced as far as this call's occurrences take it, fired or not, and
 * every gid with a bit that occurs gets its bit.  After a commit the same call
 * reports nothing.  One row named by two streams of one call gives unspecified
 * rows and hits for them, never an access outside the arrays.
 * Scratch: pm_hip_flow_seq_rules_scratch_bytes(cap, nseg), the ordered-rules
 * call's formula.  Like its siblings the call allocates nothing, never waits
 * for the host, may be captured in a graph, reads the list's cursor on the
 * device and asks the resident read_block server to leave the device first.
 * Returns 0; -1 before compile(); -2 bad arguments: the flow-rules call's
 * cases with d_prog and S for d_sets and W, and d_pos_in NULL or misaligned;
 * -12 pm_hip_set_flow_seq_rules was not called; -3 launch error.  Nothing is
 * launched or written when a check fails.  nseg == 0: returns 0 and launches
 * nothing.  cap == 0 with nseg > 0: an all-zero d_rule_ptr and untouched rows.
 * Memory safety does not depend on the data: beyond the ordered-rules call's
 * clamps a row index is tested against nrows wherever it is read, a chain-word
 * index against C and S, a bit's word against S, an index range against the
 * index array and a level against its chain's last.
 * pm_hip_flow_seq_rules: the host form, as pm_hip_flow_rules: host arrays
 * (prog updated in place, pos_in nseg u64) staged on the object's batch
 * stream; the committing call runs exactly once, behind a PM_FLOW_RULES_KEEP
 * call where its hits staging may be short; each range sorted ascending.
 * pm_flat_flow_seq_rules: the twin of the device call over host arrays, the
 * rows updated in place, each range sorted ascending; it has an index of its
 * own and does not use the device's walk; words must be the set's S; 0, or -2
 * for what the device call rejects (and a wrong words), with nothing written.
 * Measured (snort, 64 MiB in 44,740 packets of 1,500 bytes, one per flow and
 * call, two calls behind the flow scan at min_len 3, 1,000 synthetic ordered
 * rules, S = 1,020; profiles/flowseqrules/): the call alone takes 0.13-0.15 ms
 * on random ASCII (51 thousand events) and 8.2-8.3 ms on the lines stream (14.6
 * million events), 1.3-1.6x and 1.5x the ordered-rules call on the same list,
 * and 0.0074-0.019x / 0.0051-0.0054x of the list copied to the host and walked
 * by pm_flat_flow_seq_rules on one thread ("Flow ordered rules").
 */
int pm_hip_set_flow_seq_rules(void* obj, const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps,
                              size_t nrules);
size_t pm_hip_flow_seq_rule_count(void* obj);
uint32_t pm_hip_flow_seq_rules_min_len(void* obj);
uint32_t pm_hip_flow_seq_rule_words(void* obj);
uint32_t pm_hip_flow_seq_chain_count(void* obj);
int64_t pm_hip_flow_seq_chain_word(void* obj, size_t rule, uint32_t term_index);
int64_t pm_hip_flow_seq_rule_bit(void* obj, uint32_t gid);
size_t pm_hip_flow_seq_rules_scratch_bytes(uint64_t cap, int64_t nseg);
int pm_hip_flow_seq_rules_device(void* obj, const uint64_t* d_events, uint64_t cap, const unsigned long long* d_nevents,
                                 const int64_t* d_offsets, int64_t nseg, uint64_t* d_prog, int64_t nrows,
                                 const int64_t* d_rows, const uint64_t* d_pos_in, uint32_t flags, uint64_t* d_hits,
                                 uint64_t hits_cap, int64_t* d_rule_ptr, void* d_scratch, size_t scratch_bytes,
                                 void* hip_stream);
int pm_hip_flow_seq_rules(void* obj, const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                          uint64_t* prog, size_t nrows, const int64_t* rows, const uint64_t* pos_in, uint32_t flags,
                          uint64_t* hits, size_t hits_cap, int64_t* rule_ptr);
int pm_flat_flow_seq_rule_layout(const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps, size_t nrules,
                                 const uint32_t* pattern_len, size_t npat, uint32_t* chain_word_out,
                                 uint32_t* bit_by_gid_out, uint32_t* nchains_out, uint32_t* nbits_out,
                                 uint32_t* words_out);
int pm_flat_flow_seq_rules(const uint64_t* events, size_t nevents, const int64_t* offsets, size_t nseg,
                           const uint32_t* term_ptr, const uint32_t* terms, const uint32_t* gaps, size_t nrules,
                           const uint32_t* pattern_len, size_t npat, uint64_t* prog, size_t nrows, size_t words,
                           const int64_t* rows, const uint64_t* pos_in, uint32_t flags, uint64_t* hits,
                           size_t hits_cap, int64_t* rule_ptr);

/* Accuracy of one dense u32 gid stream against a reference one, on the
 * device (the scoring of Core/src/measure.c:174-190 with is_pattern_suffix,
 * PatternsTree.c:485-494): per position, equal -> success; d_algo's pattern
 * a proper suffix (ancestor) of d_real's -> partial; d_algo none -> false
 * negative; else false positive.  Also all-matches: the number of patterns
 * ending at each position of d_real (its suffix chain), summed.  Both
 * arrays come from objects compiled from the same patterns in the same add
 * order (RT and AC objects then share gids).  d_counts (5 device u64) +=
 * {success, partial, false_neg, false_pos, all_matches}.  16-B aligned.
 * Asynchronous. */
int pm_hip_score_device(void* obj, const uint32_t* d_algo, const uint32_t* d_real, int64_t n,
                        unsigned long long* d_counts, void* hip_stream);
/* Per-pattern occurrence counts of a dense u32 gid stream (all-matches
 * expansion: each position counts its answer and every pattern on the
 * answer's suffix chain).  d_hist: n_patterns + 1 device u64, indexed by gid
 * (pm_hip_gid_index maps a gid to its add order), accumulated.  Asynchronous. */
int pm_hip_pattern_counts_device(void* obj, const uint32_t* d_ids, int64_t n, unsigned long long* d_hist,
                                 void* hip_stream);
/* ac / auto kinds: keep the kernel picked for pm_hip_scan_device launches
 * (pm_hip_auto_create) for at least the next `launches` launches, so a timed
 * region never re-measures.  Returns the held kernel (1 = reverse trie,
 * 2 = AC dense rows, 3 = AC rows + records, 4 = the same with every record
 * loaded as a 16-B half, 5 = the same with deep records' 64-B blocks,
 * 6 = the same with every record as a 16-B half and two segments per lane), 0
 * when the object has no choice
 * to make (rt kind, or a single DFA form), -1 while the pick is still being
 * measured (launch more, synchronize, and ask again). */
int pm_hip_hold_choice(void* obj, int launches);
/* Before a scan_device launch is captured into a HIP graph (hipStreamBeginCapture,
 * torch.cuda.graph): allocates the scratch captured launches of the rt / auto
 * kinds use (the reverse-trie kernel's spill regions, sized for a launch of
 * any length: 512 MiB on 256 CUs), since nothing may be allocated while a
 * stream captures.  Without it a captured scan_device that would run the
 * chunked reverse-trie kernel (more than 256 Ki positions, the "rt_small_max"
 * option) returns -5 and launches nothing; smaller launches, and launches of
 * an auto object holding a DFA form, need none.  Direct launches allocate
 * their own scratch per stream (pm_hip_scratch_bytes).  0 on success. */
int pm_hip_prepare_capture(void* obj);
/* Device scratch the object holds beside its tables (pm_hip_table_bytes):
 * the capture scratch, the per-stream scratch of direct scan_device
 * launches and the read_block pipeline's staging.  Bytes. */
size_t pm_hip_scratch_bytes(void* obj);
/* Compiled-image cache: compile() keeps the flattened tables of each
 * dictionary in DIR (pm-<kind>-<hash>.img, keyed by the patterns in add order)
 * and reuses them; without a call here, $PM_IMAGE_CACHE names the directory
 * (unset = no cache).  A file that does not validate is rebuilt. */
void pm_hip_set_image_cache(void* obj, const char* dir);
/* 1 when the last compile() loaded its tables from the cache. */
int pm_hip_image_cache_hit(void* obj);
/* Start-up cost of the last compile(): *compile_ms = the whole call (gid
 * numbering, flattening or the cache read, the uploads), *upload_ms = its
 * host-to-device table copies (pm_hip_table_bytes bytes).  Wall time, ms.
 * 0, or -1 before compile().  (No reference counterpart: the reference's
 * init_mps, mps.c:109-113, is untimed.) */
int pm_hip_compile_stats(void* obj, double* compile_ms, double* upload_ms);
/* The patterns-tree parent of a gid (longest proper suffix pattern, 0 = none);
 * UINT32_MAX when out of range. */
uint32_t pm_hip_parent_gid(void* obj, uint32_t gid);

/* Device-side synthetic stream, identical to pm_gen_stream_host(). */
int pm_hip_gen_stream_device(uint8_t* d_dst, uint64_t offset, uint64_t n, uint64_t seed, int mode,
                             void* hip_stream);
void pm_gen_stream_host(uint8_t* dst, uint64_t offset, uint64_t n, uint64_t seed, int mode);
/* The "lines" stream: 1 KiB blocks of the object's patterns
 * drawn at random (splitmix64), each followed by '\n' -- dense deep matches
 * without the period of a tiled file.  Device and host give the same bytes. */
int pm_hip_gen_lines_device(void* obj, uint8_t* d_dst, uint64_t n, uint64_t seed, void* hip_stream);
void pm_gen_lines_host(void* obj, uint8_t* dst, uint64_t n, uint64_t seed);
/* The same bytes from a loaded dictionary (its patterns in first-occurrence
 * order, as pm_dict_feed adds them), without a matcher object or a device. */
struct PmDict;
void pm_gen_lines_dict(const struct PmDict* d, uint8_t* dst, uint64_t n, uint64_t seed);

uint32_t pm_hip_n_patterns(void* obj);
uint32_t pm_hip_max_pattern_len(void* obj);
/* gid (1..n) -> 0-based add_pattern order; returns UINT32_MAX if out of range */
uint32_t pm_hip_gid_index(void* obj, uint32_t gid);
/* Which kernel a compiled object runs: 1 = reverse trie, 2 = AC DFA,
 * 3 = auto (both, picked per launch). */
int pm_hip_kernel_kind(void* obj);
/* The kernel of the object's last launch: 1 = reverse trie, 2 = AC DFA
 * (0 before any). */
int pm_hip_kernel_last(void* obj);
/* DFA form of the last launch: 1 = dense rows, 2 = rows + 16-B records
 * (pm_flatten.h), 0 = the RT kernel ran. */
int pm_hip_dfa_form_last(void* obj);
/* The sparse form's kernel of the last launch that ran it ("sparse_kernel"
 * option numbering: 1 fallback-linked, 2 lock-step 8-B units, 3 lock-step
 * 16-B records; 0 before any). */
int pm_hip_sparse_kernel_last(void* obj);
/* Seconds of device time of the scan kernels issued through read_block
 * since the last reset (hipEvent based); -1 when some of those launches were
 * not timed (the "host_events" option off): the device time is then
 * unmeasured, not zero. */
double pm_hip_device_seconds(void* obj);
/* Bytes per position the last read_block's device scans wrote: 2 (u16 gids,
 * dictionaries of < 65,536 patterns, pattern-id output) or 4; 0 before any. */
int pm_hip_last_out_width(void* obj);
/* The HBM roofline every report prices against: MI355X HBM3E peak, GB/s
 * (MI355X_MICROARCH.md), shared by the CLI's CSV and bench.py. */
#define PM_HBM_PEAK_GBS 8000.0
double pm_hip_hbm_peak_gbs(void);
/* Bytes of flattened tables per kind, for DESIGN/bench reporting. */
size_t pm_hip_table_bytes(void* obj);
const char* pm_hip_last_error(void);
/* Returns the number of HIP devices (0 when none); never exits. */
int pm_hip_device_count(void);
/* hipSetDevice for C callers (the CLI's -g); 0 on success. */
int pm_hip_set_device(int device);

/* Per-object options (set before or after compile(); they change which
 * product kernel or host path the object's launches take, never a result).
 * Returns 0, or -1 for an unknown name or a value out of range.
 *   "dfa_form"        ac / auto kinds: 0 = timed choice between the DFA's
 *                     dense rows and sparse form (default), 1 = dense rows,
 *                     2 = sparse form (the pick measures again)
 *   "sparse_kernel"   the sparse form's kernel: 0 = the product choice
 *                     (default: the fallback-linked form where the object
 *                     has it), 1 = fallback-linked form, 2 = lock-step 8-B
 *                     units, 3 = lock-step 16-B records.  A forced kernel
 *                     whose image the object lacks (the FL form needs fewer
 *                     than 65,536 rows and gids, the 8-B units ids below
 *                     2^20) is not an error: the launch runs the product
 *                     choice, and pm_hip_sparse_kernel_last reports which
 *                     kernel ran
 *   "fl_hold"         the fallback-linked kernel's record loads outside the
 *                     picks' trials: 2 = deep records' 32-B blocks (0, the
 *                     default), 4 = 64-B blocks, 1 = every record as a 16-B
 *                     half (the ac / auto picks time 1 and 4, and 1 with two
 *                     chains per lane)
 *   "fl_chains"       segments per lane of the fallback-linked kernel
 *                     outside the picks' trials: 1 (0, the default) or 2
 *                     (dfa_fl2_kernel; with fl_hold 1 or 2)
 *   "dfa_sync"        1 = DFA warm-ups start at the last synchronizing 3-gram
 *                     (default), 0 = max_len - 1 bytes back
 *   "flow_seg"        the flow scan's lane segment length: 0 = the launcher's
 *                     choice (default), else a multiple of 16 in [16, 4096]
 *   "events_cap"      the device capacity, in events, of the host events
 *                     forms' first launch (pm_hip_read_*_events): 0 = the
 *                     default max(1024, n / 16); tests force the second launch
 *   "rt_small_max"    reverse-trie launches of at most this many positions
 *                     run one thread per position (-1 = default 256 Ki,
 *                     0 = never)
 *   "spill_cap_chunks" the reverse-trie spill region per wave, 1,024-position
 *                     chunks (1..16; 0 = the default fill: 4 for the count,
 *                     2 with ids -- a full region is resolved where the
 *                     other waves' streaming hides it)
 *   "host_spin" / "host_gid16" / "host_events" / "host_pool"
 *                     read_block's host path (-1 = the environment's
 *                     default, 0 / 1; csrc/pm_plugin.hip HostOpts).
 *                     host_events (default off): small read_block calls
 *                     (<= 256 Ki positions) record timing events for
 *                     pm_hip_device_seconds; the CLI turns it on
 *   "host_serve"      rt objects, and auto objects while their pick holds
 *                     the reverse trie: small read_block calls go to a resident
 *                     server grid polling a doorbell in host memory instead
 *                     of a launch per call (-1 = PM_HOST_SERVE, default 1;
 *                     0 = a launch per call).  Calls timed by host_events
 *                     take the launch path.  DESIGN.md §3
 *   "serve_idle_us"   the server grid exits after this long without a call
 *                     (-1 = PM_HOST_SERVE_IDLE_US, default 2,000; >= 10);
 *                     the next call launches it again */
int pm_hip_set_option(void* obj, const char* name, int64_t value);
/* The resident server of an rt / auto object (the "host_serve" option): grids
 * launched and requests served since the object was made.  0. */
int pm_hip_serve_stats(void* obj, uint64_t* launches, uint64_t* calls);
/* The reverse-trie kernel's streaming floor on this GPU: the same chunk
 * loop's loads and stores with no lookups (its d_out values are not match
 * ids) over d_text[0, n).  bench.py's live floor.  0 on success. */
int pm_hip_streaming_floor_device(void* obj, const uint8_t* d_text, int64_t n, void* d_out, int out_width,
                                  void* hip_stream);
/* The gather ceiling of the object's sparse DFA image (the fallback-linked
 * form; ac / auto kinds): one 1,024-lane workgroup per CU, each lane making
 * `steps` dependent 4-B loads at hashed, uniform indices over the image --
 * the deep kernel's loads without its logic, over its own table.  bench.py
 * times it beside the DFA legs: steps * 1,024 * CUs loads per launch.
 * d_sink: one device u32 (not written in practice).  0, -2 without the
 * image, -3 on a launch error. */
int pm_hip_gather_ceiling_device(void* obj, int steps, uint32_t* d_sink, void* hip_stream);
/* The read_block host path's breakdown since the last call -- out5 =
 * {staging s, enqueue s, wait s, result copy / map s, calls} -- then reset
 * and turn the accounting on (on != 0) or off.  Process-wide accounting;
 * changes no result. */
void pm_hip_host_profile(int on, double* out5);

/* ---- 3. host-only table images (no device; used by the CPU test suite
 *         to check the flattener, and by DESIGN.md sizing) ------------ */
/* kind 1 = reverse-trie image, 2 = AC dense-DFA image */
void* pm_flat_build(const char* const* pats, const uint32_t* lens, size_t n, int kind);
/* The same through the compiled-image cache in cache_dir (NULL = none). */
void* pm_flat_build_cached(const char* const* pats, const uint32_t* lens, size_t n, int kind, const char* cache_dir);
int pm_flat_cache_hit(void* handle);
int pm_flat_fits(void* handle);
/* States with full rows in the sparse DFA form (0 when it has none). */
uint32_t pm_flat_dfa_sparse_rows(void* handle);
/* name: "t12" "filt" "t3h" "rec" "next" "out" "sblock" "sout" "index_of_gid" "parent" "depth"
 * "len" (u32 bytes per gid, [0] = 0: the vector compile() uploads for the events forms);
 * returns element count */
size_t pm_flat_array(void* handle, const char* name, const void** data, size_t* elem_size);
/* read_char's host step (the per-byte path, csrc/pm_hoststep.h) over a
 * whole text from the stream start: the reverse-trie walk (RT image) or
 * the DFA step (its sparse form; dense rows when dense_rows != 0 or it has
 * none).  out_gid: n gids.  Returns 0, or -1 when the RT image does not fit. */
int pm_flat_host_scan(void* handle, const uint8_t* text, size_t n, uint32_t* out_gid, int dense_rows);
/* The flow scan's contract without a device, over the dense rows of a kind-2
 * image: the semantics of pm_hip_scan_flows_device (host arrays; state_in
 * may be NULL, state_out may be NULL or state_in; a state >=
 * pm_flat_flow_states is used as 0, and an empty stream returns its state as
 * used), and -- the image being the one compile() uploads -- the same state
 * numbers.  offsets are not checked.  Returns 0, or -1 on a kind-1 image. */
int pm_flat_host_scan_flows(void* handle, const uint8_t* text, const int64_t* offsets, size_t nseg,
                            const uint32_t* state_in, uint32_t* state_out, uint32_t* out_gid);
/* States of a kind-2 image (0 for kind 1). */
uint32_t pm_flat_flow_states(void* handle);
/* n_short: gids 1 .. n_short are exactly the patterns of <= 2 bytes (the
 * events kernels' reject without a load rests on it). */
uint32_t pm_flat_short_gids(void* handle);
/* The all-matches list (above) of n dense gids on the host, for either image
 * kind: the position is the index, the list ascends as plain u64 (position,
 * then gid), *nevents = the total, and only the first min(cap, total) events
 * are stored.  A gid out of range counts as no match.  Returns 0; -2 for
 * min_len == 0, n > 2^40, nevents NULL, or a NULL array with a non-zero
 * count; -4 with 2^24 or more patterns. */
int pm_flat_expand_matches(void* handle, const uint32_t* gids, size_t n, uint32_t min_len, uint64_t* events,
                           size_t cap, size_t* nevents);
/* Pattern groups on the host (above).  pm_flat_group_tables: from one mask
 * per pattern in add order (n = the patterns added), exactly the two arrays
 * pm_hip_set_groups uploads, n + 1 entries each in gid space with [0] = 0:
 * gmask[g] the pattern's mask, reach[g] the OR of gmask over g's suffix chain.
 * Returns 0; -2 for a wrong n or a NULL pointer.
 * pm_flat_expand_groups: the group list of n dense gids, for either image
 * kind and either form: position k lies in the stream whose offsets hold it
 * (offsets[0 .. nseg], non-decreasing; stream_groups NULL = every stream
 * 0xFFFFFFFF).  Output rules and return codes as pm_flat_expand_matches; -2
 * also for NULL groups_by_index or offsets that descend. */
int pm_flat_group_tables(void* handle, const uint32_t* groups_by_index, size_t n, uint32_t* gmask_out,
                         uint32_t* reach_out);
int pm_flat_expand_groups(void* handle, const uint32_t* gids, size_t n, const int64_t* offsets, size_t nseg,
                          const uint32_t* stream_groups, const uint32_t* groups_by_index, uint32_t min_len, int all,
                          uint64_t* events, size_t cap, size_t* nevents);
/* Pattern windows on the host (above).  pm_flat_window_tables: from
 * min_start and max_end per pattern in add order (n = the patterns added),
 * exactly the array pm_hip_set_windows uploads: 4 u32 per gid, n + 1 gids,
 *   win[4g] = need = min_start + len      win[4g+1] = max_end
 *   win[4g+2] = the minimum of need, win[4g+3] = the maximum of max_end over
 *   g's suffix chain;
 * entry 0 is { 0xFFFFFFFF, 0, 0xFFFFFFFF, 0 } (never passes; neutral for the
 * two folds).  Returns 0; -2 for a wrong n, a NULL pointer or a min_start
 * above 0x7FFFFFFF (nothing written).
 * pm_flat_expand_windows: the window list of n dense gids, for either image
 * kind and either form; pos_in NULL = every stream at byte 0; stream_groups
 * and groups_by_index may be NULL (no group tables: every pattern in every
 * group; stream_groups without groups_by_index is -2).  Output rules and
 * return codes as pm_flat_expand_groups. */
int pm_flat_window_tables(void* handle, const uint32_t* min_start_by_index, const uint32_t* max_end_by_index, size_t n,
                          uint32_t* win_out);
int pm_flat_expand_windows(void* handle, const uint32_t* gids, size_t n, const int64_t* offsets, size_t nseg,
                           const uint64_t* pos_in, const uint32_t* stream_groups, const uint32_t* groups_by_index,
                           const uint32_t* min_start_by_index, const uint32_t* max_end_by_index, uint32_t min_len,
                           int all, uint64_t* events, size_t cap, size_t* nevents);
/* Nocase on the host (above).  pm_flat_build_nocase: pm_flat_build_cached of
 * the same patterns (identical gids, and every array it serves) plus the
 * image of the folded dictionary of the same kind and the class tables for
 * the flags (one byte per pattern in add order); pm_flat_array then also
 * serves "nc_head" "nc_cnext" "nc_cword" "nc_flen" (u32), "nc_pool" "nc_flag"
 * (u8) and "nc_info" (u32 {max_chain, W, Lcs, folded patterns, folded short
 * gids, folded flow states}).
 * pm_flat_host_scan_nocase: the contract of the nocase scans over that
 * handle -- the batched semantics on a kind-1 image (state / pos / case
 * arrays ignored), the flow semantics on a kind-2 image, with the device's
 * folded state numbers and history words.  state_in / pos_in / case_in may
 * be NULL (fresh / 0 / zero), the out arrays NULL (not wanted) or the in
 * arrays themselves.  groups_by_index and the two window arrays are optional
 * (NULL: no such table; stream_groups without groups_by_index is -2).
 * Output rules and return codes as pm_flat_expand_windows; -1 on a handle of
 * pm_flat_build, or a kind-1 image that does not fit. */
void* pm_flat_build_nocase(const char* const* pats, const uint32_t* lens, const uint8_t* nocase, size_t n, int kind,
                           const char* cache_dir);
int pm_flat_host_scan_nocase(void* handle, const uint8_t* text, const int64_t* offsets, size_t nseg,
                             const uint32_t* state_in, uint32_t* state_out, const uint64_t* pos_in, uint64_t* pos_out,
                             const uint64_t* case_in, uint64_t* case_out, const uint32_t* stream_groups,
                             const uint32_t* groups_by_index, const uint32_t* min_start_by_index,
                             const uint32_t* max_end_by_index, uint32_t min_len, int all, uint64_t* events, size_t cap,
                             size_t* nevents);
void pm_flat_free(void* handle);

#ifdef __cplusplus
}
#endif
#endif /* PM_HIP_H */
