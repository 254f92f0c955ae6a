"""Step a recorded plan op by op on the GPU and compare what each kernel
really reads and writes with the boxes ``hazards.footprint`` declares for it
(tests/test_gpu_footprints.py).

The watch set is every device storage reachable from the engine and the plan
(the walk of ``hazards.live_ranges``), viewed as int32 words.  ``P`` is the
replay-written part of it: the write boxes of all ops plus the host-written
inputs MIX and NZ.  The storages P touches (and the engine's status words)
are "hot": they are snapshotted, poisoned and restored as one flat word
vector.  All other storages -- weights, tables, unused workspaces -- are
"cold": no box declares them written, so each op must leave every word of
them as it was.

For op i with (R, W) = footprint(op, d), from the state S0 its predecessors
left:

* write check -- run it: every word that changed lies in a box of W (the
  status words are exempt, and zero after the run);
* read check -- restore S0, overwrite every word of P outside R and W with a
  poison, run it again: the W boxes and the status words hold the same bits
  as after the clean run.  Twice: a NaN word (as f32 and as two f16 halves),
  which survives a multiply by a zero mask, and a finite 1e30 pattern, which
  survives a select that drops NaNs.

Poison is data only: index, tag and length memory (GRU granules, counts,
K-slice workspaces) is written by its op and so never poisoned for it.
"""
import bisect
import ctypes
import struct

import torch

from open_universe_amd import _lib as L
from open_universe_amd import hazards as H
from open_universe_amd.bundle import pointer_fields

SYNC = (L.OP_LANE, L.OP_SIGNAL, L.OP_WAIT)
KIND_NAMES = {v: k[3:] for k, v in vars(L).items() if k.startswith("OP_") and isinstance(v, int)}
POISONS = (("nan", 0x7FC07E00), ("1e30", struct.unpack("<i", struct.pack("<f", 1e30))[0]))
SMALL_WORDS = 1 << 18   # cold storages below this many words are compared as one concatenation


def storages(device, *roots):
    """data_ptr -> untyped storage of every tensor on ``device`` reachable
    from ``roots`` (attributes, dicts, lists, tuples: hazards.live_ranges' walk)."""
    seen, out, stack = set(), {}, list(roots)
    while stack:
        o = stack.pop()
        if id(o) in seen or o is None or isinstance(o, (int, float, str, bytes, bool)):
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            st = o.untyped_storage()
            if st.nbytes() and o.device == device:
                out[st.data_ptr()] = st
            continue
        if isinstance(o, dict):
            stack.extend(o.values())
        elif isinstance(o, (list, tuple, set)):
            stack.extend(o)
        elif hasattr(o, "__dict__") and not isinstance(o, type):
            stack.extend(vars(o).values())
    return out


def inputs(plan, mix_src, seed=1028282):
    """A fixed (mix, noise) for ``plan``: ``mix_src`` (items, 1, >= T) cropped
    and tiled to the plan's batch, noise from a seeded CPU generator."""
    mix = torch.as_tensor(mix_src, dtype=torch.float32)[:, :, :plan.mix_len]
    assert mix.shape[-1] == plan.mix_len
    mix = mix.repeat(-(-plan.B // mix.shape[0]), 1, 1)[:plan.B].contiguous()
    g = torch.Generator().manual_seed(seed)
    nz = torch.stack([torch.randn((plan.B, 1, plan.Tp), generator=g) for _ in range(plan.NZ.shape[0])])
    return mix.to(plan.dev), nz.to(plan.dev)


class Report:
    def __init__(self):
        self.failures = []      # (op index, kind, check, fields, text)
        self.ops = 0            # recorded ops checked
        self.words = 0          # tile-word variants checked
        self.refused = 0        # tile-word variants ou_conv refused (-2)
        self.kinds = set()      # op kinds checked
        self.tiles = []         # (fir mode, prec, tile word) of every variant checked

    def __str__(self):
        return "\n".join(f[-1] for f in self.failures)


class Stepper:
    """See the module docstring.  ``hazards.footprint`` is looked up at every
    call, so a test can monkeypatch a mutant over it.  ``run`` stops after
    ``limit`` failures; a Report holds them, each naming the op index, label
    and kind, the descriptor field nearest to the offending bytes and those
    bytes relative to it."""

    def __init__(self, eng, plan, limit=4):
        self.eng, self.plan, self.limit = eng, plan, limit
        self.dev = plan.NZ.device
        self.lib = L.load()
        self.kinds = plan.prog.op_kinds()
        self.descs = plan.prog.descs
        self.labels = plan.prog.labels
        st = sorted(storages(self.dev, eng, plan).items())
        self.base = [p for p, _ in st]
        self.end = [p + s.nbytes() for p, s in st]
        assert all(e <= b for e, b in zip(self.end, self.base[1:])), "watched storages overlap"
        self.view = []
        for p, s in st:
            assert p % 4 == 0 and s.nbytes() % 4 == 0, ("a watched storage is not made of 4-byte words", p, s.nbytes())
            self.view.append(torch.empty(0, dtype=torch.uint8, device=self.dev).set_(s).view(torch.int32))
        # ---- P, the hot storages and their flat word space
        pboxes = [b for op, d in zip(self.kinds, self.descs) if op not in SYNC for b in self.fp(op, d)[1]]
        pboxes += [H.Box(t.data_ptr(), 0, 0, 1, 1, 0, t.numel() * 4) for t in (plan.MIX, plan.NZ)]
        sbox = H.Box(eng.status.data_ptr(), 0, 0, 1, 1, 0, eng.status.numel() * 4)
        hot = sorted({self.find(b) for b in pboxes + [sbox]})
        self.off, n = {}, 0
        for k in hot:
            self.off[k] = n
            n += self.view[k].numel()
        self.hot, self.n = hot, n
        self.hot_starts = [self.off[k] for k in hot]
        self.hot_views = [self.view[k] for k in hot]
        self.P = torch.zeros(n, dtype=torch.bool, device=self.dev)
        for b in pboxes:
            self.strided(self.P, b).fill_(True)
        self.status = torch.zeros(n, dtype=torch.bool, device=self.dev)
        self.strided(self.status, sbox).fill_(True)
        self.Wm = torch.zeros(n, dtype=torch.bool, device=self.dev)     # the current op's W (cleared after it)
        self.keep = torch.zeros(n, dtype=torch.bool, device=self.dev)   # the current op's R and W
        # ---- the cold storages: a snapshot of each, the small ones also as one vector
        cold = [k for k in range(len(st)) if k not in self.off]
        self.snap = {k: self.view[k].clone() for k in cold}
        # compared one by one: the large ones, and the K-slice workspace at any size (a tile word with K
        # slices declares a part of it written, which is then left out of the comparison)
        alone = {k for k in cold if self.view[k].numel() >= SMALL_WORDS}
        alone |= {self.find(H.Box(eng.ks_ws.data_ptr(), 0, 0, 1, 1, 0, 4))} & set(cold)
        self.small = [k for k in cold if k not in alone]
        self.big = [k for k in cold if k in alone]
        self.small_snap = torch.cat([self.snap[k] for k in self.small]) if self.small else None
        self.S = torch.cat(self.hot_views)   # the live state of the hot words

    # ------------------------------------------------------------ addresses
    def fp(self, op, d):
        return H.footprint(op, d, self.lib)

    def find(self, b):
        """Index of the watched storage that holds the whole of box ``b``."""
        k = bisect.bisect_right(self.base, b.lo) - 1
        assert k >= 0 and b.hi <= self.end[k], f"box {b} lies in no watched storage"
        return k

    def strided(self, mask, b):
        """The words of box ``b`` (in a hot storage) as a view of ``mask``."""
        for v in (b.base + b.t0, b.t1 - b.t0, b.bs, b.cs):
            assert v % 4 == 0, f"box {b} is not 4-byte aligned"
        k = self.find(b)
        nb, nc = (b.nb if b.bs else 1), (b.nc if b.cs else 1)
        return mask.as_strided((nb, nc, (b.t1 - b.t0) // 4), (b.bs // 4, b.cs // 4, 1),
                               self.off[k] + (b.lo - self.base[k]) // 4)

    def address(self, flat, extras):
        """Byte address of flat word index ``flat``."""
        if flat >= self.n:
            flat -= self.n
            for k, lo, hi in extras:
                if flat < hi - lo:
                    return self.base[k] + 4 * (lo + flat)
                flat -= hi - lo
        j = bisect.bisect_right(self.hot_starts, flat) - 1
        return self.base[self.hot[j]] + 4 * (flat - self.hot_starts[j])

    def fields(self, d):
        """(name, pointer) of every non-null pointer field of descriptor d."""
        blob = bytes(d)
        out = [(name, struct.unpack_from("<Q", blob, off)[0]) for name, off in pointer_fields(type(d))]
        return [(n, p) for n, p in out if p]

    def nearest(self, d, boxes, addr):
        """The pointer field whose box (or, without one, whose address) is
        nearest to byte address ``addr``: (name, pointer, its boxes)."""
        best = None
        for name, p in self.fields(d):
            bx = [b for b in boxes if b.base == p]
            lo, hi = (min(b.lo for b in bx), max(b.hi for b in bx)) if bx else (p, p + 4)
            dist = 0 if lo <= addr < hi else min(abs(addr - lo), abs(addr - hi + 1))
            if best is None or dist < best[0]:
                best = (dist, name, p, bx)
        return best[1:] if best else ("?", addr, [])

    def describe(self, i, op, d, what, check, addrs, boxes):
        addrs = addrs or [0]
        name, p, bx = self.nearest(d, boxes, addrs[0])
        rel = ", ".join(f"{a - p:+d}" for a in addrs[:6])
        return (name, f"op {i} ({self.labels[i]!r}, {KIND_NAMES.get(op, op)}{what}): {check}: nearest field {name} "
                      f"= {p:#x}, boxes {bx}; offending bytes relative to it: {rel}")

    # ------------------------------------------------------------ state
    def read(self, extras):
        return torch.cat(self.hot_views + [self.view[k][lo:hi] for k, lo, hi in extras])

    def write(self, flat, extras):
        dst = self.hot_views + [self.view[k][lo:hi] for k, lo, hi in extras]
        torch._foreach_copy_(dst, list(flat.split([v.numel() for v in dst])))

    def cold_dirty(self, extras):
        """0-dim bool tensors, one per comparison, and what each compared."""
        flags, what = [], []
        if self.small:
            flags.append((torch.cat([self.view[k] for k in self.small]) != self.small_snap).any())
            what.append(self.small)
        for k in self.big:
            cuts = sorted((lo, hi) for kk, lo, hi in extras if kk == k)
            pos = 0
            for lo, hi in cuts + [(self.view[k].numel(), 0)]:
                if lo > pos:
                    flags.append((self.view[k][pos:lo] != self.snap[k][pos:lo]).any())
                    what.append([k])
                pos = max(pos, hi)
        return flags, what

    def cold_addresses(self, ks, extras):
        out = []
        for k in ks:
            diff = self.view[k] != self.snap[k]
            for kk, lo, hi in extras:
                if kk == k:
                    diff[lo:hi] = False
            out += [self.base[k] + 4 * int(j) for j in diff.nonzero()[:6, 0].tolist()]
        return out

    def settle(self, inputs, junk=0x3DCCCCCD, strict=True):
        """Before stepping, after the plan has been replayed whole: the
        replays must have left the cold storages as they were when this
        Stepper was made, and every word of P outside the ``inputs`` tensors is
        overwritten with ``junk`` (a finite value as f32 and as f16 halves), so
        that no op finds the bits it is about to write already in place: a
        write outside W then always shows, also from an op whose output no
        later op overwrites, and the closing check starts from a wrong output.
        Not ``strict`` (a test's mutated footprint): cold storages the replays
        changed are filled with junk as well instead of failing here."""
        flags, ks_of = self.cold_dirty([])
        got = torch.stack(flags).tolist() if flags else []
        dirty = [ks for f, ks in zip(got, ks_of) if f]
        assert not (dirty and strict), ("replaying the plan changed storages no op declares written, first bytes at",
                                        [hex(a) for ks in dirty for a in self.cold_addresses(ks, [])][:6])
        for k in (k for ks in dirty for k in ks):   # not strict (a mutated footprint): junk there too
            self.view[k].fill_(junk)
            self.snap[k] = self.view[k].clone()
        if dirty and self.small:
            self.small_snap = torch.cat([self.snap[k] for k in self.small])
        m = self.P.clone()
        for t in inputs:
            self.strided(m, H.Box(t.data_ptr(), 0, 0, 1, 1, 0, t.numel() * 4)).fill_(False)
        self.S = torch.where(m, torch.tensor(junk, dtype=torch.int32, device=self.dev), self.read([]))
        self.write(self.S, [])

    # ------------------------------------------------------------ one op
    def check(self, rep, i, op, d, launch, advance, what="", cold=True):
        """Write check and read check of one launch from the live state;
        leaves the state after the launch (advance) or as it was.  Returns
        False when the launch was refused (-2, nothing checked).  cold=False
        leaves the comparison of the cold storages to the caller (they are
        never restored, so a later cold_check still sees a stray write)."""
        R, W = self.fp(op, d)
        marked, extras = [], []
        for b in R + W:
            k = self.find(b)
            if k in self.off:
                marked.append(self.strided(self.keep, b))
                if any(b is w for w in W):
                    marked.append(self.strided(self.Wm, b))
            elif any(b is w for w in W):   # a write box in a cold storage (a K-slice workspace): watched for this op
                assert k in self.big and b.lo % 4 == 0 and b.hi % 4 == 0, (
                    f"op {i} ({self.labels[i]!r}{what}): write box {b} lies in a storage no recorded op writes "
                    "and that is not the K-slice workspace, or is not 4-byte aligned")
                extras.append((k, (b.lo - self.base[k]) // 4, (b.hi - self.base[k]) // 4))
        for m in marked:
            m.fill_(True)
        ne = sum(hi - lo for _, lo, hi in extras)
        pad = (lambda m, v: torch.cat([m, torch.full((ne,), v, dtype=torch.bool, device=self.dev)])) if ne else \
            (lambda m, v: m)
        Wm, status = pad(self.Wm, True), pad(self.status, False)
        poison = pad(self.P & ~self.keep, False)
        S0 = self.S if not ne else torch.cat([self.S] + [self.snap[k][lo:hi] for k, lo, hi in extras])
        fail = lambda check, addrs, boxes: rep.failures.append(   # noqa: E731
            (i, op, check) + self.describe(i, op, d, what, check, addrs, boxes))
        try:
            rc = launch()
            if rc == -2:
                return False
            assert rc == 0, (i, self.labels[i], rc, self.lib.ou_last_error())
            S1 = self.read(extras)
            bad = (S1 != S0) & ~(Wm | status)
            flags, ks_of = self.cold_dirty(extras) if cold else ([], [])
            got = torch.stack([bad.any(), ((S1 != 0) & status).any()] + flags).tolist()
            if got[0]:
                fail("write check (a changed word outside W)",
                     [self.address(int(j), extras) for j in bad.nonzero()[:6, 0].tolist()], W)
            if got[1]:
                j = ((S1 != 0) & status).nonzero()[:6, 0].tolist()
                fail("status words not zero after the clean run", [self.address(int(x), extras) for x in j], W)
            self.cold_failures(fail, got[2:], ks_of, extras, W)
            for pname, pword in POISONS:
                pword = torch.tensor(pword, dtype=torch.int32, device=self.dev)
                self.write(torch.where(poison, pword, S0), extras)
                assert launch() == 0
                S2 = self.read(extras)
                bad = (S2 != S1) & (Wm | status)
                if bool(bad.any()):
                    addrs = [self.address(int(j), extras) for j in bad.nonzero()[:6, 0].tolist()]
                    fail(f"read check ({pname} poison outside R and W changes the result)", addrs, W)
                    self.culprits(rep, i, op, d, launch, S0, S1, poison, Wm | status, pword, extras, R + W, what)
                    break
            self.S = (S1 if advance else S0)[:self.n]
            self.write(self.S, [])
            for k, lo, hi in extras:   # a cold storage goes back to its snapshot either way
                self.view[k][lo:hi].copy_(self.snap[k][lo:hi])
            return True
        finally:
            for m in marked:
                m.fill_(False)

    def cold_failures(self, fail, flags, ks_of, extras, W, who=""):
        for f, ks in zip(flags, ks_of):
            if f:
                fail("write check (a constant changed%s)" % who, self.cold_addresses(ks, extras), W)
                for k in ks:
                    self.view[k].copy_(self.snap[k])

    def cold_check(self, rep, i, op, d, who):
        """The cold storages against their snapshots, after launches checked with cold=False."""
        flags, ks_of = self.cold_dirty([])
        if flags and any(torch.stack(flags).tolist()):
            fail = lambda check, addrs, boxes: rep.failures.append(   # noqa: E731
                (i, op, check) + self.describe(i, op, d, "", check, addrs, boxes))
            self.cold_failures(fail, torch.stack(flags).tolist(), ks_of, [], self.fp(op, d)[1], who)

    def culprits(self, rep, i, op, d, launch, S0, S1, poison, watch, pword, extras, boxes, what):
        """After a failed read check: poison one hot storage at a time and name
        the pointer fields into the storages whose poison changes the result."""
        by_k = {}
        for name, p in self.fields(d):
            k = bisect.bisect_right(self.base, p) - 1
            if k >= 0 and p < self.end[k] and k in self.off:
                by_k.setdefault(k, []).append((name, p))
        for k, names in by_k.items():
            lo, hi = self.off[k], self.off[k] + self.view[k].numel()
            part = torch.zeros_like(poison)
            part[lo:hi] = poison[lo:hi]
            if not bool(part.any()):
                continue
            self.write(torch.where(part, pword, S0), extras)
            assert launch() == 0
            if bool(((self.read(extras) != S1) & watch).any()):
                addrs = [self.address(int(j), extras) for j in part.nonzero()[:6, 0].tolist()]
                name, p = min(names, key=lambda np_: abs(np_[1] - addrs[0]))
                bx = [b for b in boxes if b.base == p]
                rel = ", ".join(f"{a - p:+d}" for a in addrs)
                rep.failures.append((i, op, "read culprit", "/".join(n for n, _ in names),
                                     f"op {i} ({self.labels[i]!r}, {KIND_NAMES.get(op, op)}{what}): reads undeclared "
                                     f"bytes of the buffer of {'/'.join(n for n, _ in names)}: boxes of {name} {bx}; "
                                     f"first poisoned bytes relative to it: {rel}"))

    # ------------------------------------------------------------ the plan
    def run(self, kinds=None, variants=None):
        """Step the whole program.  ``kinds``: check only ops of these kinds
        (the others just run).  ``variants(i, d)``: further descriptors of conv
        op i to check from the same state ([(tile word, ConvDesc)])."""
        rep = Report()
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        tuner, hook = L.TUNER, L.ADD_HOOK
        L.TUNER = L.ADD_HOOK = None   # the descriptors go out exactly as recorded
        try:
            for i, (op, d) in enumerate(zip(self.kinds, self.descs)):
                if op in SYNC:
                    continue
                prog = L.Program()
                prog.add(op, d)

                def launch(prog=prog):
                    prog.run(stream)
                    return 0

                if kinds is not None and op not in kinds:
                    launch()
                    self.S = None
                    continue
                if self.S is None:
                    self.S = self.read([])
                if variants is not None and op == L.OP_CONV:
                    swept = rep.words
                    for word, dv in variants(i, d):
                        ok = self.check(rep, i, op, dv, lambda dv=dv: self.lib.ou_conv(ctypes.byref(dv),
                                                                                      ctypes.c_void_p(stream)),
                                        False, what=f", tile word {word:#x}", cold=False)
                        rep.words += ok
                        rep.refused += not ok
                        if ok:
                            rep.tiles.append((dv.fir, dv.prec, word))
                    if rep.words > swept:
                        self.cold_check(rep, i, op, d, " under one of this geometry's tile words")
                self.check(rep, i, op, d, launch, True)
                rep.ops += 1
                rep.kinds.add(op)
                if len(rep.failures) >= self.limit:
                    break
        finally:
            L.TUNER, L.ADD_HOOK = tuner, hook
        torch.cuda.synchronize(self.dev)
        return rep
