"""Inputs and oracle answers of the flow-scan tests (test_flows.py on the GPU,
test_flows_cpu.py without one).  TEST INFRASTRUCTURE.

Input F: 1 MiB of dictionary patterns drawn at random, each followed by a
newline (batch_inputs.t_text's recipe), as 256 flows of 4,096 bytes.  Every
flow is cut into packets: first the 16 edge lengths (0 also in a run, 1..5,
15/16/17 around a 16-byte block, 63/64/65, 255/256/257) rotated by the flow's
number, then random lengths below 300 until its 4,096 bytes are used.  Call r
holds packet r of every flow, in flow order; a flow that has run out
contributes an empty stream.  Dense deep matches straddle most packet
boundaries, so a scan that answers every packet from its own first byte
differs from the per-flow answers at thousands of positions, many of them well
inside their packet.
"""
import numpy as np

from oracle_lib import oracle_for

F_FLOWS = 256
F_FLOW_BYTES = 4096
F_BYTES = F_FLOWS * F_FLOW_BYTES
F_HEAD_LENGTHS = [0, 1, 2, 3, 0, 0, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257]

_cache = {}


def f_text(key, n=F_BYTES):
    pats = [p[2] for p in oracle_for(key).patterns()]
    rng = np.random.default_rng(5)
    parts, total = [], 0
    while total < n:
        p = pats[rng.integers(0, len(pats))] + b"\n"
        parts.append(p)
        total += len(p)
    return np.frombuffer(b"".join(parts)[:n], dtype=np.uint8).copy()


def f_packets():
    """Per flow, the offsets of its packets inside its 4,096 bytes (int64,
    0 first, 4,096 last)."""
    rng = np.random.default_rng(11)
    flows = []
    for f in range(F_FLOWS):
        lengths = np.roll(F_HEAD_LENGTHS, f).tolist()
        total = sum(lengths)
        while total < F_FLOW_BYTES:
            k = int(rng.integers(0, 300))
            lengths.append(k)
            total += k
        offs = np.zeros(len(lengths) + 1, dtype=np.int64)
        np.cumsum(lengths, out=offs[1:])
        flows.append(np.minimum(offs, F_FLOW_BYTES))
    return flows


class InputF:
    """text: the 1 MiB; flows[f]: flow f's packet offsets; calls: a list of
    (data, offsets, expected codes), one per call, stream f of a call being
    flow f's packet (empty once the flow has run out); exp: the codes of the
    whole text, every flow scanned from its own first byte."""

    def __init__(self, key):
        self.key = key
        self.text = f_text(key)
        self.flows = f_packets()
        o = oracle_for(key)
        self.exp = np.zeros(F_BYTES, dtype=np.uint32)
        for f in range(F_FLOWS):
            o.reset()
            self.exp[f * F_FLOW_BYTES:(f + 1) * F_FLOW_BYTES] = o.scan_codes(
                self.text[f * F_FLOW_BYTES:(f + 1) * F_FLOW_BYTES])
        o.reset()
        self.ncalls = max(len(p) - 1 for p in self.flows)
        self.calls = []
        for r in range(self.ncalls):
            spans = self.spans(r)
            data = np.concatenate([self.text[a:b] for a, b in spans] + [np.zeros(0, np.uint8)])
            exp = np.concatenate([self.exp[a:b] for a, b in spans] + [np.zeros(0, np.uint32)])
            offs = np.zeros(F_FLOWS + 1, dtype=np.int64)
            np.cumsum([b - a for a, b in spans], out=offs[1:])
            for a in (data, offs, exp):
                a.setflags(write=False)
            self.calls.append((data, offs, exp))
        for a in (self.text, self.exp):
            a.setflags(write=False)

    def spans(self, r):
        """[a, b) in the text of packet r of every flow (a == b: none left)."""
        out = []
        for f, p in enumerate(self.flows):
            base = f * F_FLOW_BYTES
            out.append((base + int(p[r]), base + int(p[r + 1])) if r + 1 < len(p) else (base + F_FLOW_BYTES,) * 2)
        return out


def input_f(key):
    """Input F of a dictionary; cached, callers do not modify it."""
    if key not in _cache:
        _cache[key] = InputF(key)
    return _cache[key]


def precondition(key):
    """(positions whose per-flow answer differs from the answer of a scan that
    resets at every packet, those of them 8 or more bytes into their packet)."""
    F = input_f(key)
    o = oracle_for(key)
    differ = deep = 0
    for f, p in enumerate(F.flows):
        base = f * F_FLOW_BYTES
        for a, b in zip(p[:-1].tolist(), p[1:].tolist()):
            if b > a:
                o.reset()
                got = o.scan_codes(F.text[base + a:base + b])
                d = np.nonzero(got != F.exp[base + a:base + b])[0]
                differ += int(d.size)
                deep += int(np.count_nonzero(d >= 8))
    o.reset()
    return differ, deep


def shape_figures():
    """(calls, fewest packets of a flow, empty packets before the run-outs)."""
    flows = f_packets()
    return (max(len(p) - 1 for p in flows), min(len(p) - 1 for p in flows),
            sum(int(np.count_nonzero(np.diff(p) == 0)) for p in flows))
