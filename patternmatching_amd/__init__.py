"""patternmatching_amd -- MI355X-native streaming multi-pattern matcher.

A drop-in for the per-byte matcher path of yehonatan145/PatternMatching
(the ``mps_table`` plugin interface, Core/src/mps.h:71-80, driven by the
``-d/-s`` stream loop of Core/src/measure.c:241-311).  The scan runs in
hand-written HIP kernels for gfx950 (``csrc/pm_kernels.hip``) behind a
C-ABI (``include/pm_hip.h``); this package is the Python host mirror of that
interface:

    Dictionary      Core/src/PatternsTree.c:260-312 + parser.c:63-99
    HipMatcher      one MpsElem instance (create / add_pattern / compile /
                    read_char / read_block / reset / total_mem / free)
    gen_stream      the synthetic stream specification
    batch_offsets   the offsets array of a list of streams, for the batched
                    scan (HipMatcher.read_batch_* / scan_batch_device)
    FlowTable       flow key -> carried state over the flow scan
                    (HipMatcher.read_flows_* / scan_flows_device)
    unpack_events   (positions, gids) of the match list the events forms of
                    both scans give (HipMatcher.read_*_events /
                    scan_*_events_device) and, with every pattern that
                    ends at a position, their all-matches forms
                    (HipMatcher.read_*_matches / scan_*_matches_device,
                    FlowTable.scan_matches), and their group forms: a group
                    mask per pattern (HipMatcher.set_groups) and per stream
                    (HipMatcher.read_*_groups / scan_*_groups_device,
                    FlowTable.scan_groups), and their window forms: where in
                    its stream a pattern may lie, Snort's offset and depth
                    (HipMatcher.set_windows, read_*_windows /
                    scan_*_windows_device, FlowTable.scan_windows), and their
                    nocase forms: a case-insensitivity flag per pattern,
                    Snort's nocase (HipMatcher.set_nocase, read_*_nocase /
                    scan_*_nocase_device, FlowTable.scan_nocase)
    events_by_stream_host   any such list grouped by stream without a device
                    (the host twin of HipMatcher.events_by_stream /
                    events_by_stream_device / read_many_sets: per-stream
                    ranges, optionally one event per stream and pattern)
    rules_by_stream_host    which multi-pattern rules (positive and negated
                    terms, pack_rules) fire in each stream of such a list,
                    without a device (the host twin of HipMatcher.set_rules /
                    rules_by_stream / rules_by_stream_device / read_many_rules)
    flow_rules_host         the rules whose terms lie in different packets of a
                    flow: a set of carried terms per flow, the rules that
                    become true in each call, without a device (the host twin
                    of HipMatcher.set_flow_rules / flow_rules /
                    flow_rules_device and FlowTable.scan_rules;
                    flow_rule_bits_host gives the sets' bit numbering)
    seq_rules_by_stream_host    ordered rules (pack_seq_rules: terms that must
                    follow one another at a distance, Snort's distance:N)
                    without a device (the host twin of
                    HipMatcher.set_seq_rules / seq_rules_by_stream /
                    seq_rules_by_stream_device / read_many_seq_rules)
    flow_seq_rules_host     ordered rules (distance only) whose terms lie in
                    different packets of a flow: a progress row per flow, the
                    rules that become true in each call, without a device (the
                    host twin of HipMatcher.set_flow_seq_rules / flow_seq_rules
                    / flow_seq_rules_device and FlowTable.scan_seq_rules;
                    flow_seq_rule_layout_host gives the rows' layout)
"""
from ._lib import load, LIB_PATH, CLI_PATH  # noqa: F401
from .matcher import (  # noqa: F401
    Dictionary,
    HipMatcher,
    FlowTable,
    gen_stream,
    batch_offsets,
    unpack_events,
    events_by_stream_host,
    BY_STREAM_UNIQUE,
    pack_rules,
    rules_by_stream_host,
    flow_rules_host,
    flow_rule_bits_host,
    pack_seq_rules,
    pack_seq_rules_within,
    seq_rules_by_stream_host,
    flow_seq_rules_host,
    flow_seq_rule_layout_host,
    SEQ_FREE,
    FLOW_RULES_KEEP,
    RULE_NEGATED,
    RULE_FAST,
    parse_line,
    KIND_RT,
    KIND_AC,
    KIND_AUTO,
)

__all__ = ["load", "Dictionary", "HipMatcher", "FlowTable", "gen_stream", "batch_offsets", "unpack_events", "parse_line",
           "events_by_stream_host", "BY_STREAM_UNIQUE", "pack_rules", "rules_by_stream_host",
           "flow_rules_host", "flow_rule_bits_host", "pack_seq_rules", "pack_seq_rules_within",
           "seq_rules_by_stream_host", "flow_seq_rules_host", "flow_seq_rule_layout_host", "SEQ_FREE",
           "FLOW_RULES_KEEP", "RULE_NEGATED", "RULE_FAST", "KIND_RT", "KIND_AC", "KIND_AUTO", "LIB_PATH", "CLI_PATH"]
