"""Test-only replay of the engine's launch trace (include/fhe_rocm.h, fhe_ctx_trace): what Engine::flush, lincomb
and the eager ops enqueue on the stream, in that order, evaluated again here by references that share no code with
the product.  Never used by the product.

  parse             the flat u64 stream -> Level (with its Nodes) / Lincomb / Write records
  check_structure   every source written earlier (a Write, a Lincomb, a Node of a strictly earlier level); within a
                    level no destination twice and no destination that is also a source of that level; level numbers
                    consecutive; node counts equal to fhe_ctx_level_log, their total to the fhe_ctx_stats delta
  replay_plain      address -> plaintext (in half message steps), updated in trace order; a node's input is
                    sum coef * value + cst / delta, must lie in its table's domain, its output is the table entry --
                    the table rebuilt from fhe_ctx_lut_table by the restatement of the table kinds below
  replay_words      address -> 2049 words; a node's input is the wrapping u64 combination (ks_ref.lincomb_np's arithmetic), then
                    the oracle's keyswitch, ms_center_ref in centered mode, the oracle's blind rotation under the
                    polynomial lut_poly() builds from the table entries, the oracle's sample extraction

The plaintext replay cannot see a coefficient that is wrong but congruent (an input that stays inside the table's
domain and happens to hit an equal entry); the word replay can."""
import ctypes as C
from collections import deque

import numpy as np

LEVEL, NODE, LINCOMB, WRITE = 1, 2, 3, 4
WRITE_UPLOAD, WRITE_DEFERRED, WRITE_OPAQUE = 0, 1, 2
LUT_INTEGER, LUT_HALF_STEP, LUT_OPRF = 0, 1, 2
LEVEL_SPLIT = 1 << 31
MSG_CARRY = 16
DELTA = (1 << 63) // MSG_CARRY
N = 2048
BIG_CT = N + 1
M64 = (1 << 64) - 1


class ReplayError(AssertionError):
    pass


def _i64(v):
    v = int(v)
    return v - (1 << 64) if v >> 63 else v


class Node:
    __slots__ = ("dst", "lut", "cst", "terms")

    def __init__(self, dst, lut, cst, terms):
        self.dst, self.lut, self.cst, self.terms = dst, lut, cst, terms

    def __repr__(self):
        return f"Node(dst={self.dst:#x}, lut={self.lut}, cst={self.cst:#x}, terms={[(hex(s), c) for s, c in self.terms]})"


class Lincomb(Node):
    pass


class Level:
    __slots__ = ("number", "split", "nodes")

    def __init__(self, number, split, nodes):
        self.number, self.split, self.nodes = number, split, nodes


class Write:
    __slots__ = ("kind", "addrs")

    def __init__(self, kind, addrs):
        self.kind, self.addrs = kind, addrs


def parse(words):
    """the records of a trace, in order; a malformed stream raises"""
    w = words.tolist() if isinstance(words, np.ndarray) else [int(x) for x in words]
    out, i = [], 0

    def op(i, with_lut):
        dst = w[i + 1]
        lut = w[i + 2] if with_lut else None
        j = i + (3 if with_lut else 2)
        cst, nt = w[j], w[j + 1]
        if nt > 64 or j + 2 + 2 * nt > len(w):
            raise ReplayError(f"trace: a record of {nt} terms at word {i}")
        seg = w[j + 2:j + 2 + 2 * nt]
        terms = list(zip(seg[0::2], map(_i64, seg[1::2])))
        return dst, lut, cst, terms, j + 2 + 2 * nt

    while i < len(w):
        tag = w[i]
        if tag == LEVEL:
            number, count, split = w[i + 1], w[i + 2], w[i + 3]
            i += 4
            nodes = []
            for _ in range(count):
                if i >= len(w) or w[i] != NODE:
                    raise ReplayError(f"trace: level {number} announces {count} nodes, {len(nodes)} follow")
                dst, lut, cst, terms, i = op(i, True)
                nodes.append(Node(dst, lut, cst, terms))
            out.append(Level(number, bool(split), nodes))
        elif tag == LINCOMB:
            dst, _, cst, terms, i = op(i, False)
            out.append(Lincomb(dst, None, cst, terms))
        elif tag == WRITE:
            kind, n = w[i + 1], w[i + 2]
            if i + 3 + n > len(w):
                raise ReplayError(f"trace: a write of {n} addresses at word {i}")
            out.append(Write(kind, w[i + 3:i + 3 + n]))
            i += 3 + n
        else:
            raise ReplayError(f"trace: tag {tag} at word {i} (a node outside a level?)")
    return out


def unparse(records):
    """the u64 stream of records (the mutation tests edit records and replay them)"""
    w = []
    for r in records:
        if isinstance(r, Level):
            w += [LEVEL, r.number, len(r.nodes), int(r.split)]
            for n in r.nodes:
                w += [NODE, n.dst, n.lut, n.cst, len(n.terms)] + [x & M64 for t in n.terms for x in t]
        elif isinstance(r, Lincomb):
            w += [LINCOMB, r.dst, r.cst, len(r.terms)] + [x & M64 for t in r.terms for x in t]
        else:
            w += [WRITE, r.kind, len(r.addrs)] + list(r.addrs)
    return np.array(w, np.uint64)


def nodes_of(records):
    return [n for r in records if isinstance(r, Level) for n in r.nodes]


def check_structure(records, level_log=None, pbs=None):
    """the launch order is a valid execution of some dependency graph, and the bookkeeping counts what was launched"""
    written = set()
    last = None
    for r in records:
        if isinstance(r, Write):
            written.update(r.addrs)
        elif isinstance(r, Lincomb):
            for s, _ in r.terms:
                if s not in written:
                    raise ReplayError(f"lincomb into {r.dst:#x} reads {s:#x}, which nothing has written")
            if any(s == r.dst for s, _ in r.terms):
                raise ReplayError(f"lincomb into its own source {r.dst:#x}")
            written.add(r.dst)
        else:
            if last is not None and r.number != last + 1:
                raise ReplayError(f"level {r.number} follows level {last}")
            last = r.number
            srcs = set()
            for n in r.nodes:
                if n.dst == 0:
                    raise ReplayError(f"level {r.number}: a node without a destination")
                for s, _ in n.terms:
                    if s not in written:
                        raise ReplayError(f"level {r.number}: {n!r} reads {s:#x}, which no write, lincomb or earlier "
                                          "level has written")
                    srcs.add(s)
            dsts = [n.dst for n in r.nodes]
            if len(set(dsts)) != len(dsts):
                raise ReplayError(f"level {r.number}: a destination written twice")
            both = srcs.intersection(dsts)
            if both:
                raise ReplayError(f"level {r.number}: {sorted(map(hex, both))[:4]} read and written in one level")
            written.update(dsts)
    levels = [r for r in records if isinstance(r, Level)]
    if level_log is not None:
        got = [len(r.nodes) | (LEVEL_SPLIT if r.split else 0) for r in levels]
        if got != [int(x) for x in level_log]:
            raise ReplayError(f"trace levels {got[:8]}.. ({len(got)}) != level_log {list(level_log)[:8]}.. ({len(level_log)})")
    if pbs is not None and sum(len(r.nodes) for r in levels) != pbs:
        raise ReplayError(f"{sum(len(r.nodes) for r in levels)} traced nodes, fhe_ctx_stats counts {pbs}")


# ------------------------------------------------------------------------------------------ the table kinds
def table_value(kind, entries, half2):
    """output (half message steps) of a table on an input given in half message steps; outside its domain raises.
    The torus holds 32 message steps (16 of message and carry, doubled by the padding bit), so an input is what it
    is mod 64 half steps: the engine's constants arrive reduced so (a negative constant wraps in the u64 body)."""
    if half2 % 2:
        raise ReplayError(f"a lookup input off the message grid: {half2} half steps")
    if kind == LUT_INTEGER:  # f over [0, 16), outputs mod 16; [16, 32) is the padding bit's half
        v = half2 % (4 * MSG_CARRY) // 2
        if v >= MSG_CARRY:
            raise ReplayError(f"a lookup input outside the message space: {v} (of 32 steps on the torus)")
        return 2 * (entries[v] % MSG_CARRY)
    if kind == LUT_HALF_STEP:  # 16 signed outputs in half steps over [0, 16); [-16, 0) is the negacyclic half
        v = ((half2 + 2 * MSG_CARRY) % (4 * MSG_CARRY) - 2 * MSG_CARRY) // 2
        return entries[v] if v >= 0 else -entries[v + MSG_CARRY]
    raise ReplayError(f"a launched level cannot use a table of kind {kind}")


def lut_poly(kind, entries, make_lut=None, delta=DELTA):
    """the accumulator polynomial (2048 u64) of a table: an integer table by the oracle's make_lut, the half-step
    table from its definition -- box i of 128 coefficients holds entries[i] half steps (signed), the whole rotated
    by half a box with the wrapped half box negated -- and the staircase by tests/oprf_ref.py"""
    if kind == LUT_INTEGER:
        return np.asarray(make_lut([e % MSG_CARRY for e in entries]), np.uint64)
    if kind == LUT_HALF_STEP:
        box = N // MSG_CARRY
        flat = [(entries[j // box] * (delta // 2)) & M64 for j in range(N)]
        rot = [flat[j + box // 2] if j + box // 2 < N else (-flat[j + box // 2 - N]) & M64 for j in range(N)]
        return np.array(rot, np.uint64)
    if kind == LUT_OPRF:
        import oprf_ref
        return oprf_ref.lut(entries[0], delta)
    raise ReplayError(f"table kind {kind}")


# ------------------------------------------------------------------------------------------ plaintext replay
class Inputs:
    """what the program's own writes put at an address, in write order (a recycled slot is written again)"""

    def __init__(self):
        self.q = {}

    def note(self, addrs, values):
        for a, v in zip(addrs, values):
            if a:
                self.q.setdefault(a, deque()).append(v)

    def take(self, addr):
        q = self.q.get(addr)
        return q.popleft() if q else None  # None: an opaque write, unknown to the replay


def digits(value, nblocks):
    return [(value >> (2 * k)) & 3 for k in range(nblocks)]


def replay_plain(records, tables, inputs, delta=DELTA):
    """address -> plaintext in half message steps after the whole trace; tables: id -> (kind, entries); inputs: an
    Inputs of 2 x the block values.  Also returns the number of addresses written more than once."""
    val, rewritten = {}, 0

    def read(n):
        c2, rem = divmod(_i64(n.cst), delta // 2)
        if rem:
            raise ReplayError(f"{n!r}: constant off the half-step grid")
        acc = c2
        for s, coef in n.terms:
            if val.get(s) is None:
                raise ReplayError(f"{n!r} reads {s:#x}, whose value the replay does not know")
            acc += coef * val[s]
        return acc

    for r in records:
        if isinstance(r, Write):
            for a in r.addrs:
                rewritten += a in val
                val[a] = inputs.take(a)
        elif isinstance(r, Lincomb):
            rewritten += r.dst in val
            val[r.dst] = read(r)
        else:
            outs = []
            for n in r.nodes:
                kind, entries = tables[n.lut]
                try:
                    outs.append(table_value(kind, entries, read(n)))
                except ReplayError as e:
                    raise ReplayError(f"level {r.number}: {n!r}: {e}") from None
            for n, o in zip(r.nodes, outs):
                rewritten += n.dst in val
                val[n.dst] = o
    return val, rewritten


def value_of(val, addrs, trivial, bits):
    """sum block 4^k mod 2^bits of a value's blocks (fhe_*_block_addrs) under a plaintext map"""
    total = 0
    for k, (a, t) in enumerate(zip(addrs, trivial)):
        if a == 0:
            v = t
        else:
            h2 = val.get(a)
            if h2 is None or h2 % 2 or h2 < 0:
                raise ReplayError(f"result block {k} at {a:#x}: {h2} half steps")
            v = h2 // 2
        total += v << (2 * k)
    return total % (1 << bits)


# ------------------------------------------------------------------------------------------ word replay
def replay_words(records, tables, inputs, ok, centered=False):
    """address -> 2049 u64 words after the whole trace, every launched node evaluated through the oracle `ok`
    (oracle.OracleKeys under the device's keys).  inputs: an Inputs of rows.  Returns (map, rewritten)."""
    import ms_center_ref
    import oracle

    lib = oracle.load()
    n_small = ok.params.n
    polys = {}

    def poly(lut):
        if lut not in polys:
            polys[lut] = lut_poly(*tables[lut], make_lut=ok.make_lut, delta=ok.delta())
        return polys[lut]

    val, rewritten = {}, 0

    def combine(n):
        acc = np.zeros(BIG_CT, np.uint64)
        with np.errstate(over="ignore"):
            for s, coef in n.terms:
                if val.get(s) is None:
                    raise ReplayError(f"{n!r} reads {s:#x}, whose words the replay does not know")
                acc += np.uint64(coef & M64) * val[s]
            acc[N] += np.uint64(n.cst)
        return acc

    for r in records:
        if isinstance(r, Write):
            for a in r.addrs:
                rewritten += a in val
                val[a] = inputs.take(a)
        elif isinstance(r, Lincomb):
            rewritten += r.dst in val
            val[r.dst] = combine(r)
        else:
            ins = np.stack([combine(n) for n in r.nodes])
            ids = sorted({n.lut for n in r.nodes})
            luts = np.stack([poly(i) for i in ids])
            idx = np.array([ids.index(n.lut) for n in r.nodes], np.uint32)
            if not centered:
                outs = ok.pbs_batch(ins, luts, idx)
            else:
                small = ms_center_ref.center_ref(ok.keyswitch_batch(ins), n_small)
                outs = np.zeros_like(ins)
                glwe = np.zeros(2 * N, np.uint64)
                u64p = C.POINTER(C.c_uint64)
                for g in range(len(r.nodes)):
                    row = np.ascontiguousarray(small[g, :n_small + 1])
                    lib.fho_blind_rotate(ok.ref, row.ctypes.data_as(u64p), np.ascontiguousarray(luts[idx[g]]).ctypes.data_as(u64p),
                                         glwe.ctypes.data_as(u64p))
                    lib.fho_sample_extract(glwe.ctypes.data_as(u64p), outs[g].ctypes.data_as(u64p))
            for g, n in enumerate(r.nodes):
                rewritten += n.dst in val
                val[n.dst] = outs[g].copy()
    return val, rewritten


# ------------------------------------------------------------------------------------------ a traced program
class Recorder:
    """Trace on over a context for the time of one program: note() the operands as they are encrypted, finish()
    reads the trace, holds it to the level log and the statistics, and returns the records with the tables of
    every LUT id they name."""

    def __init__(self, ctx):
        import fhe_sign as F
        self.F, self.ctx = F, ctx
        self.inputs = Inputs()
        F.level_log(ctx, reset=True)
        self.pbs0 = F.stats(ctx)[0]
        F.trace_read(ctx, reset=True)
        F.trace_enable(ctx, True)

    def addrs(self, x):
        return self.F.block_addrs(self.ctx, x)

    def note(self, x, value):
        """a freshly encrypted operand holding `value` (plaintext replay: 2 x its digits)"""
        a, _ = self.addrs(x)
        self.inputs.note(a, [2 * d for d in digits(value, len(a))])
        return x

    def note_rows(self, x, rows):
        """the same for the word replay: the operand's exported rows"""
        a, _ = self.addrs(x)
        self.inputs.note(a, [np.array(r, np.uint64) for r in rows])
        return x

    def finish(self, eager_pbs=0):
        """eager_pbs: bootstraps of eager ops (random values, decompressions), which fhe_ctx_stats counts and no level holds"""
        F = self.F
        F.trace_enable(self.ctx, False)
        records = parse(F.trace_read(self.ctx, reset=True))
        check_structure(records, F.level_log(self.ctx, reset=True), F.stats(self.ctx)[0] - self.pbs0 - eager_pbs)
        tables = {i: F.lut_table(self.ctx, i) for i in sorted({n.lut for n in nodes_of(records)})}
        return records, tables

    def close(self):
        self.F.trace_enable(self.ctx, False)
