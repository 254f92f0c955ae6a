"""Exported enhance bundles: a recorded :class:`~open_universe_amd.plan.EnhancePlan`
as a relocatable file, and its replay through the model-level C ABI.

An ``EnhancePlan`` is a flat ``ou_program``: a list of descriptors whose only
process-specific content is device addresses.  :func:`export_bundle` records
the plan for one ``(batch, length, options)``, settles its exponents and tiles
with one run, and writes the descriptors with every pointer turned into a
``(region, offset)`` relocation, next to the bytes of every constant the
descriptors reach (include/ouhip.h has the file layout).  ``ou_bundle_load``
rebuilds the program in any process -- :class:`Bundle` here, or a C host
(examples/enhance_host.cpp) -- without weight folding, packing, tile tuning or
recording, and without Python.

:class:`Bundle` needs torch only for the tensors its caller passes; it
imports neither the engine nor the recorder.
"""
import bisect
import ctypes
import json
import os
import struct
from ctypes import c_void_p

from . import _lib as L

MAGIC = b"OUHB"
FORMAT_VERSION = 1
ARCH = "gfx950"
HEADER_BYTES, REGION_ENT, OP_ENT, RELOC_ENT, IO_ENT = 128, 32, 64, 24, 32
KIND_ARENA, KIND_SAVED, KIND_ZERO = 0, 1, 2

_UNSUPPORTED = ("ensemble", "ensemble_stat", "use_aux_signal", "warm_start", "target", "fake_score_snr")


def pointer_fields(st, base=0, prefix=""):
    """(name, byte offset) of every pointer-typed field of a descriptor
    structure of _lib.py, nested structures and pointer arrays included."""
    for name, typ in st._fields_:
        off = base + getattr(st, name).offset
        if typ is c_void_p:
            yield prefix + name, off
        elif issubclass(typ, ctypes.Array) and typ._type_ is c_void_p:
            for k in range(typ._length_):
                yield f"{prefix}{name}[{k}]", off + 8 * k
        elif issubclass(typ, ctypes.Structure):
            yield from pointer_fields(typ, off, prefix + name + ".")


def fnv1a(data, h=0xCBF29CE484222325):
    """64-bit FNV-1a (the checksum of the header and tables)."""
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _align(n, a=64):
    return (n + a - 1) // a * a


class Exported:
    """What :func:`export_bundle` wrote: ``path``, the recorded ``plan`` (and
    its ``engine``, which owns the constants), ``regions`` [(lo, hi, kind)] in
    region order at the recording process's addresses, ``relocs`` [(op, byte
    offset in the descriptor, region, offset in the region)] and the
    ``file_bytes``."""

    def __init__(self, path, plan, engine, regions, relocs, file_bytes):
        self.path, self.plan, self.engine = path, plan, engine
        self.regions, self.relocs, self.file_bytes = regions, relocs, file_bytes


def _storages(*roots):
    """data_ptr -> untyped storage of every torch tensor reachable from
    ``roots`` (the walk of hazards.live_ranges, keeping the storages)."""
    import torch

    seen, out, stack = set(), {}, list(roots)
    while stack:
        o = stack.pop()
        if id(o) in seen or o is None or isinstance(o, (int, float, str, bytes, bool)):
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            st = o.untyped_storage()
            if st.nbytes():
                out[st.data_ptr()] = st
            continue
        if isinstance(o, dict):
            stack.extend(o.values())
        elif isinstance(o, (list, tuple, set)):
            stack.extend(o)
        elif hasattr(o, "__dict__") and not isinstance(o, type):
            stack.extend(vars(o).values())
    return out


def _storage_bytes(st):
    import torch

    return torch.empty(0, dtype=torch.uint8, device=st.device).set_(st).cpu().numpy().tobytes()


def write_plan(eng, plan, path, meta):
    """Serialise a recorded EnhancePlan (see the module docstring); ``meta``
    is the JSON blob.  Returns an :class:`Exported`."""
    from . import hazards as H

    lib = L.load()
    prog = plan.prog
    kinds, descs = prog.op_kinds(), prog.descs
    assert len(kinds) == len(descs) == len(prog.labels)
    if plan.arena is None or getattr(plan, "RED", None) is not None:
        raise NotImplementedError("export_bundle: a plain EnhancePlan recorded onto an arena")
    live = sorted(set(H.live_ranges(eng, plan)))
    starts = [a for a, _ in live]

    def find(p):
        k = bisect.bisect_right(starts, p) - 1
        return live[k] if k >= 0 and live[k][0] <= p < live[k][1] else None

    ast = plan.arena.buf.untyped_storage()
    arena = (ast.data_ptr(), ast.data_ptr() + ast.nbytes())
    # every non-null pointer field of every op -> the tensor storage it points into
    raw, used = [], {arena}
    for i, (op, d) in enumerate(zip(kinds, descs)):
        blob = bytes(d)
        for name, off in pointer_fields(type(d)):
            p = struct.unpack_from("<Q", blob, off)[0]
            if not p:
                continue
            r = find(p)
            if r is None:
                raise L.OuHipError(f"export_bundle: op {i} ({prog.labels[i]!r}): {type(d).__name__}.{name} = {p:#x} "
                                   "points into no tensor of the engine or the plan")
            used.add(r)
            raw.append((i, off, r, p - r[0]))
    n_status = 4 + len(eng.range_owners)
    io_ptrs = [(plan.MIX.data_ptr(), 0, plan.B, plan.mix_len), (plan.NZ.data_ptr(), plan.n_noise, plan.B, plan.Tp),
               (plan.OUT.data_ptr(), 0, plan.B, plan.mix_len), (eng.status.data_ptr(), n_status, 0, 0)]
    for p, *_ in io_ptrs:
        r = find(p)
        assert r is not None, "an I/O buffer of the plan is not reachable from it"
        used.add(r)
    order = [arena] + sorted(used - {arena})
    rid = {r: k for k, r in enumerate(order)}
    # a region some op writes starts zeroed at load instead of being saved
    # (K-slice workspaces, GRU granules; the status words always)
    ostarts = [a for a, _ in order[1:]]
    written = {find(eng.status.data_ptr())}
    for op, d in zip(kinds, descs):
        if op in (L.OP_LANE, L.OP_SIGNAL, L.OP_WAIT):
            continue
        if op == L.OP_CONV and d.ks_ws:   # a conv whose tile is picked at launch (-1) may still K-slice
            written.add(find(d.ks_ws))
        for b in H.footprint(op, d, lib)[1]:
            k = max(0, bisect.bisect_right(ostarts, b.lo) - 1)
            while k < len(ostarts) and order[1 + k][0] < b.hi:
                if order[1 + k][1] > b.lo:
                    written.add(order[1 + k])
                k += 1
    kind = {r: KIND_ARENA if r == arena else KIND_ZERO if r in written else KIND_SAVED for r in order}
    stor = _storages(eng, plan)

    # ---- layout: header | regions | ops | relocations | I/O | descriptors | JSON | saved bytes
    js = json.dumps(meta, sort_keys=True).encode("utf-8")
    r_off = HEADER_BYTES
    o_off = _align(r_off + REGION_ENT * len(order))
    l_off = _align(o_off + OP_ENT * len(kinds))
    io_off = _align(l_off + RELOC_ENT * len(raw))
    d_off = _align(io_off + 4 * IO_ENT)
    d_offs, pos = [], d_off
    for d in descs:
        d_offs.append(pos)
        pos += _align(ctypes.sizeof(d), 8)
    j_off = _align(pos)
    meta_end = _align(j_off + len(js))
    pos = meta_end
    p_offs = {}
    for r in order:
        if kind[r] == KIND_SAVED:
            p_offs[r] = pos
            pos = _align(pos + r[1] - r[0])
    file_bytes = pos

    body = bytearray(meta_end)
    for k, r in enumerate(order):
        struct.pack_into("<IIQQQ", body, r_off + REGION_ENT * k, kind[r], 0, r[1] - r[0], p_offs.get(r, 0), 0)
    relocs, first = [], 0
    by_op = {}
    for i, off, r, roff in raw:
        by_op.setdefault(i, []).append((off, rid[r], roff))
    for i, (op, d) in enumerate(zip(kinds, descs)):
        mine = sorted(by_op.get(i, []))
        blob = bytearray(bytes(d))
        for off, _, _ in mine:
            blob[off:off + 8] = bytes(8)
        body[d_offs[i]:d_offs[i] + len(blob)] = blob
        label = prog.labels[i].encode("utf-8")[:39]
        struct.pack_into("<IIQII40s", body, o_off + OP_ENT * i, op, len(blob), d_offs[i], first, len(mine), label)
        for off, region, roff in mine:
            struct.pack_into("<IIIIQ", body, l_off + RELOC_ENT * len(relocs), i, off, region, 0, roff)
            relocs.append((i, off, region, roff))
        first += len(mine)
    for k, (p, count, b, t) in enumerate(io_ptrs):
        r = find(p)
        struct.pack_into("<IIQIIQ", body, io_off + IO_ENT * k, rid[r], count, p - r[0], b, t, 0)
    body[j_off:j_off + len(js)] = js
    struct.pack_into("<4sIIIIIII16sQQQQQQ", body, 0, MAGIC, FORMAT_VERSION, L.ABI_VERSION, len(order), len(kinds),
                     len(relocs), len(js), 0, ARCH.encode(), r_off, o_off, l_off, io_off, j_off, file_bytes)
    struct.pack_into("<Q", body, 104, meta_end)
    struct.pack_into("<Q", body, 96, fnv1a(body[HEADER_BYTES:meta_end], fnv1a(body[:96])))
    with open(path, "wb") as f:
        f.write(body)
        for r in order:
            if kind[r] != KIND_SAVED:
                continue
            f.seek(p_offs[r])
            data = _storage_bytes(stor[r[0]])
            assert len(data) == r[1] - r[0]
            f.write(data)
        f.truncate(file_bytes)
    return Exported(path, plan, eng, [(r[0], r[1], kind[r]) for r in order], relocs, file_bytes)


def record_plan(model, eng, batch, length, n_steps, epsilon, keep_rms):
    """The EnhancePlan on a fresh arena of its own (slot 0, the st lane on)."""
    from . import engine as E
    from .plan import EnhancePlan

    size = 64 << 20
    while True:
        try:
            return EnhancePlan(eng, batch, length, n_steps, epsilon, keep_rms=keep_rms, diff=dict(model.diff_kwargs),
                               slot=0, arena=E.Arena(eng.device, size), st_lane=True)
        except E.ArenaFull as e:
            size = max(2 * size, int(e.args[0] * 1.5))


def export_bundle(model, path, batch, length, n_steps=None, epsilon=None, keep_rms=False, calib=None, name=None,
                  **options):
    """Record ``model.enhance`` for ``batch`` clips of ``length`` samples and
    write it to ``path`` as a bundle.  On a HIP device the plan runs once on
    ``calib`` (a (batch, length) clip; default: synthetic speech-like audio):
    a split-f16 range error goes through the model's recovery as in
    ``enhance``, and the plan that ran clean is the one exported, so the
    file's exponents and tiles are settled.  A model on the CPU is recorded
    without running (no GPU needed; tiles are then picked at load).
    Ensembles, the aux signal, warm starts and the known-answer mode are not
    exportable.  Returns an :class:`Exported`."""
    import torch

    for k in options:
        if k in _UNSUPPORTED:
            raise NotImplementedError(f"export_bundle: {k} is not supported in a bundle")
        raise TypeError(f"export_bundle() got an unexpected keyword argument {k!r}")
    n_steps = int(model.diff_kwargs.n_steps if n_steps is None else n_steps)
    epsilon = float(model.diff_kwargs.epsilon if epsilon is None else epsilon)
    batch, length, keep_rms = int(batch), int(length), bool(keep_rms)
    dev = next(model.parameters()).device
    if dev.type == "cuda":
        from .utils.synthetic import synth_audio

        if calib is None:
            import numpy as np

            calib = torch.from_numpy(np.stack([synth_audio(length, model.fs, i)[0] for i in range(batch)]))
        mix = calib.to(dev, torch.float32).reshape(batch, 1, length).contiguous()
        plan = record_plan(model, model._get_engine(), batch, length, n_steps, epsilon, keep_rms)
        with torch.no_grad():
            try:
                plan(mix, torch.Generator(device=dev).manual_seed(0))
            except L.OuRangeError as e:
                nz = plan.NZ.clone()
                del plan
                got = []

                def rerun():   # the exponents are read at record time: record again, run on the same noise
                    got[:] = [record_plan(model, model._get_engine(), batch, length, n_steps, epsilon, keep_rms)]
                    return got[0].run_with_noise(mix, nz)

                model._range_recover(e, rerun)
                plan = got[0]
        eng = plan.eng
    else:
        from .engine import Engine

        eng = Engine(model._model_cfg(), model.state_dict(), "cpu", _record_only=True)
        plan = record_plan(model, eng, batch, length, n_steps, epsilon, keep_rms)
    meta = {"fs": int(model.fs), "n_steps": n_steps, "epsilon": epsilon, "keep_rms": keep_rms,
            "conv_prec": int(eng.conv_prec), "config": name or type(model).__name__}
    return write_plan(eng, plan, path, meta)


def randn(n, seed, offset=0, device="cuda"):
    """``n`` values of the native noise stream (ou_randn) as a device tensor."""
    import torch

    out = torch.empty(int(n), dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        L.check(L.load().ou_randn(out.data_ptr(), int(n), int(seed), int(offset),
                                  c_void_p(torch.cuda.current_stream(out.device).cuda_stream)), "randn")
    return out


def _io(io):
    return {"region": io.region, "count": io.count, "offset": io.offset, "batch": io.batch, "length": io.length}


class Bundle:
    """A loaded bundle on the current HIP device (ou_bundle_load): every
    region allocated and filled, the program rebuilt and, with ``capture``,
    captured as one hipGraph.  Calls on one Bundle are not re-entrant."""

    def __init__(self, path, capture=True):
        self.lib = L.load()
        self.h = c_void_p()
        L.check(self.lib.ou_bundle_load(os.fsencode(path), int(bool(capture)), ctypes.byref(self.h)), "bundle_load")
        m = L.BundleMeta()
        L.check(self.lib.ou_model_info(self.h, ctypes.byref(m)), "model_info")
        self.batch, self.length = m.mix.batch, m.mix.length
        self.n_noise, self.padded_length = m.noise.count, m.noise.length
        self.info = dict(json.loads(m.json.decode("utf-8")), batch=self.batch, length=self.length,
                         n_noise=self.n_noise, padded_length=self.padded_length, n_ops=m.n_ops,
                         n_regions=m.n_regions, region_bytes=m.region_bytes, status_words=m.status.count,
                         arch=m.arch.decode(), capture=bool(capture))

    def _mix(self, mix):
        import torch

        if not mix.is_cuda or mix.dtype != torch.float32 or mix.numel() != self.batch * self.length:
            raise ValueError(f"mix must be a float32 HIP tensor of {self.batch} x {self.length} samples")
        mix = mix.contiguous()
        out = torch.empty((self.batch, self.length), dtype=torch.float32, device=mix.device)
        return mix, out, c_void_p(torch.cuda.current_stream(mix.device).cuda_stream)

    def enhance_with_noise(self, mix, noise):
        """One enhance on the caller's noise, a float32 HIP tensor of
        n_noise x batch x padded_length values (x0 first, then one z per
        intermediate step).  Returns (batch, length); call status() before
        using it."""
        mix, out, stream = self._mix(mix)
        if (not noise.is_cuda or noise.dtype != mix.dtype
                or noise.numel() != self.n_noise * self.batch * self.padded_length):
            raise ValueError(f"noise must be a float32 HIP tensor of {self.n_noise} x {self.batch} x "
                             f"{self.padded_length} values")
        noise = noise.contiguous()
        L.check(self.lib.ou_model_enhance_noise(self.h, mix.data_ptr(), noise.data_ptr(), out.data_ptr(), stream),
                "model_enhance_noise")
        return out

    def enhance(self, mix, seed=0, offset=0):
        """One enhance on the native noise stream at (seed, offset)."""
        mix, out, stream = self._mix(mix)
        L.check(self.lib.ou_model_enhance(self.h, mix.data_ptr(), out.data_ptr(), int(seed), int(offset), stream),
                "model_enhance")
        return out

    def long_noise(self, n, overlap):
        """(floats of the global noise buffer, L) of a windowed enhance of an
        ``n``-sample clip: ``n_noise`` draws of ``L`` values (longform.py)."""
        ln = ctypes.c_int64(0)
        total = self.lib.ou_model_long_noise(self.h, int(n), int(overlap), ctypes.byref(ln))
        if total < 0:
            L.check(int(total), "model_long_noise")
        return int(total), int(ln.value)

    def _long(self, x):
        import torch

        if not x.is_cuda or x.dtype != torch.float32 or x.ndim != 1:
            raise ValueError("x must be a one-dimensional float32 HIP tensor")
        x = x.contiguous()
        return x, torch.empty_like(x), c_void_p(torch.cuda.current_stream(x.device).cuda_stream)

    def enhance_long_with_noise(self, x, overlap, noise):
        """Windowed enhance (longform.py) of one clip ``x`` of more than
        ``length`` samples: windows of the bundle's ``length``, ``overlap``
        samples crossfaded, groups of the bundle's ``batch`` windows per
        replay, on the caller's global noise of n_noise x L values
        (``long_noise``).  Returns (n,); call status() before using it."""
        x, out, stream = self._long(x)
        total, _ = self.long_noise(x.numel(), overlap)
        if not noise.is_cuda or noise.dtype != x.dtype or noise.numel() != total:
            raise ValueError(f"noise must be a float32 HIP tensor of {total} values")
        noise = noise.contiguous()
        L.check(self.lib.ou_model_enhance_long_noise(self.h, x.data_ptr(), x.numel(), int(overlap), noise.data_ptr(),
                                                     out.data_ptr(), stream), "model_enhance_long_noise")
        return out

    def enhance_long(self, x, overlap, seed=0, offset=0):
        """The same on the native noise stream: draw k is ou_randn at
        (seed, counter offset + k ceil(L / 4))."""
        import torch

        x, out, stream = self._long(x)
        total, _ = self.long_noise(x.numel(), overlap)
        ws = torch.empty(total, dtype=torch.float32, device=x.device)
        L.check(self.lib.ou_model_enhance_long(self.h, x.data_ptr(), x.numel(), int(overlap), out.data_ptr(),
                                               int(seed), int(offset), ws.data_ptr(), stream), "model_enhance_long")
        return out

    def stream(self, overlap, seed=0, offset=0):
        """A streaming session on this bundle (:class:`BundleStream`): one at
        a time, and ``enhance*`` is refused while it is open."""
        return BundleStream(self, overlap, seed, offset)

    def stream_mux(self, overlap, channels):
        """A mux session on this bundle (:class:`BundleMux`): ``channels``
        streams share the slots of its plan.  One session at a time -- a mux
        or a stream -- and ``enhance*`` is refused while it is open."""
        return BundleMux(self, overlap, channels)

    def status(self):
        """Wait for the latest enhance and read the status words: 0 when it
        ran clean; raises OuHipError on a GRU hand-off timeout and
        OuRangeError when a split-f16 operand left its range (the output is
        then undefined: use a bundle exported with f32 operands)."""
        rc = self.lib.ou_model_status(self.h)
        if rc == 0:
            return 0
        msg = (self.lib.ou_last_error() or b"").decode()
        raise (L.OuRangeError if rc == 2 else L.OuHipError)(f"bundle: {msg}")

    def close(self):
        if getattr(self, "h", None):
            for s in (getattr(self, "_stream", None), getattr(self, "_mux", None)):
                if s is not None:
                    s.release()
            self.lib.ou_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BundleStream:
    """A streaming session through the C ABI (ou_model_stream_*; DESIGN.md
    section 15): ``push(x) -> Tensor`` takes the next samples of the stream (a
    CPU or device tensor, any length) and returns the samples that became final
    on the device; ``close() -> Tensor`` returns the rest; ``bound(n)`` is the
    count ``push`` of ``n`` samples would return, ``bound(closing=True)`` what
    ``close`` would.  The window and the group size are the bundle's ``length``
    and ``batch``.  A context manager: leaving it destroys the session.  Call
    the bundle's ``status()`` before using what a push returned."""

    def __init__(self, bundle, overlap, seed=0, offset=0):
        self.bundle, self.lib = bundle, bundle.lib
        self.h = c_void_p()
        L.check(self.lib.ou_model_stream_open(bundle.h, int(overlap), int(seed), int(offset), ctypes.byref(self.h)),
                "model_stream_open")
        bundle._stream = self

    def _raise(self, rc, what):
        from .longform import StreamShort

        msg = (self.lib.ou_last_error() or b"").decode()
        if rc == L.STREAM_SHORT:
            raise StreamShort(f"{what}: {msg}")
        raise (L.OuRangeError if rc == 2 else L.OuHipError)(f"{what}: ouhip error {rc}: {msg}")

    def bound(self, n=0, closing=False):
        r = self.lib.ou_model_stream_bound(self.h, int(n), int(bool(closing)))
        if r < 0:
            self._raise(L.STREAM_SHORT if closing else int(r), "model_stream_bound")
        return int(r)

    def _out(self, n):
        import torch

        dev = torch.device("cuda", torch.cuda.current_device())
        return torch.empty(n, dtype=torch.float32, device=dev), c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def push(self, x):
        import torch

        x = torch.as_tensor(x)
        if x.ndim != 1 and x.numel() != x.shape[-1]:
            raise ValueError("a stream is one mono signal: push (n,), (1, n) or (1, 1, n)")
        out, stream = self._out(self.bound(x.numel()))
        x = x.reshape(-1).to(device=out.device, dtype=torch.float32).contiguous()
        got = ctypes.c_int64(0)
        rc = self.lib.ou_model_stream_push(self.h, x.data_ptr() if x.numel() else 0, x.numel(),
                                           out.data_ptr() if out.numel() else 0, ctypes.byref(got), stream)
        if rc:
            self._raise(rc, "model_stream_push")
        assert got.value == out.numel(), (got.value, out.numel())
        return out

    def close(self):
        n = self.lib.ou_model_stream_bound(self.h, 0, 1)
        out, stream = self._out(max(int(n), 0))
        got = ctypes.c_int64(0)
        rc = self.lib.ou_model_stream_close(self.h, out.data_ptr() if out.numel() else 0, ctypes.byref(got), stream)
        if rc:
            self._raise(rc, "model_stream_close")
        assert got.value == out.numel(), (got.value, out.numel())
        return out

    def release(self):
        if getattr(self, "h", None):
            self.lib.ou_model_stream_destroy(self.h)
            self.h = None
            if getattr(self.bundle, "_stream", None) is self:
                self.bundle._stream = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class BundleMux:
    """A mux session through the C ABI (ou_model_mux_*),
    with the interface of ``mux.ModelMux``: ``open(seed, offset, channel) ->
    c``, ``room(c)``, ``push(c, x)`` (a CPU or device tensor of at most
    ``room(c)`` samples), ``close(c)``, ``run(full_only) ->`` one device tensor
    per channel (views of one buffer), ``bound(full_only) -> (counts,
    offsets)``.  The window and the batch are the bundle's ``length`` and
    ``batch``.  A context manager: leaving it destroys the session.  Call the
    bundle's ``status()`` before using what a run returned."""

    def __init__(self, bundle, overlap, channels):
        self.bundle, self.lib, self.channels = bundle, bundle.lib, int(channels)
        self.h = c_void_p()
        L.check(self.lib.ou_model_mux_open(bundle.h, int(overlap), self.channels, ctypes.byref(self.h)),
                "model_mux_open")
        bundle._mux = self

    def _check(self, rc, what):
        from .longform import StreamShort

        if rc == 0:
            return
        msg = (self.lib.ou_last_error() or b"").decode()
        if rc == L.STREAM_SHORT:
            raise StreamShort(f"{what}: {msg}")
        raise (L.OuRangeError if rc == 2 else L.OuHipError)(f"{what}: ouhip error {rc}: {msg}")

    def open(self, seed=0, offset=0, channel=None):
        got = ctypes.c_int(-1)
        self._check(self.lib.ou_model_mux_channel_open(self.h, -1 if channel is None else int(channel), int(seed),
                                                       int(offset), ctypes.byref(got)), "model_mux_channel_open")
        return got.value

    def room(self, c):
        r = self.lib.ou_model_mux_room(self.h, int(c))
        if r < 0:
            self._check(int(r), "model_mux_room")
        return int(r)

    def push(self, c, x):
        import torch

        x = torch.as_tensor(x)
        if x.ndim != 1 and x.numel() != x.shape[-1]:
            raise ValueError("a stream is one mono signal: push (n,), (1, n) or (1, 1, n)")
        dev = torch.device("cuda", torch.cuda.current_device())
        x = x.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
        self._check(self.lib.ou_model_mux_push(self.h, int(c), x.data_ptr() if x.numel() else 0, x.numel(),
                                               c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                    "model_mux_push")

    def close(self, c):
        self._check(self.lib.ou_model_mux_close(self.h, int(c)), "model_mux_close")

    def bound(self, full_only=False):
        counts, offsets = (ctypes.c_int64 * self.channels)(), (ctypes.c_int64 * self.channels)()
        self._check(self.lib.ou_model_mux_bound(self.h, int(bool(full_only)), counts, offsets), "model_mux_bound")
        return list(counts), list(offsets)

    def run(self, full_only=False):
        import torch

        counts, offsets = self.bound(full_only)
        dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty(sum(counts), dtype=torch.float32, device=dev)
        got = (ctypes.c_int64 * self.channels)()
        self._check(self.lib.ou_model_mux_run(self.h, int(bool(full_only)), out.data_ptr() if out.numel() else 0, got,
                                              c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "model_mux_run")
        assert list(got) == counts, (list(got), counts)
        return [out[o:o + n] for o, n in zip(offsets, counts)]

    def release(self):
        if getattr(self, "h", None):
            self.lib.ou_model_mux_destroy(self.h)
            self.h = None
            if getattr(self.bundle, "_mux", None) is self:
                self.bundle._mux = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
