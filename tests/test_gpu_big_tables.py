"""GPU: the table-indexing HIP kernels on one table past 4 GiB (G1, G1-QR: byte offsets past 2^31 and 2^32) and on
one past 2^31 floats (G2: element offsets past 2^31, byte offsets past 2^33).  tests/big_table_cases.py has the
geometries, probed rows and batches, and says which kind of truncation each geometry can witness;
tests/test_big_table_cases.py asserts those claims on the CPU, holds the twin to the float64 oracle and runs the host
kernels.

Relocation equivalence, bit for bit.  The huge model's one big table holds model values in K <= 64 probed rows and
POISON = 1024 everywhere else; the twin has that table compacted to the K rows and its indices remapped by the monotone
map row -> rank.  The same kernel on the same route does the same arithmetic on both, so every comparison below is
torch.equal / np.array_equal with no tolerance -- logits, the probed rows' gradients, parameters and optimizer state --
followed by the complement: after the probed rows are zeroed the gradient buffer has no non-zero element, after they
are re-poisoned every element of the table is POISON, and the moments are zero outside them (a write to a wrong row,
which no read-side check sees).  The deterministic routes run the `dup` batch (B = 37, the rows at the crossings hit
twice or more) and `once` (every probed row exactly once); the atomic routes are asserted on `once`, where every
gradient row of the huge table has a single addend, and on the huge field's rows only.

Routes.  Inference on G1 (4.3 GB table, 6.9 GB / 3.4 GB / 1.7 GB serving copies; on dup, the reversed dup and once):
both f32 kernels (DFWFM_DIAG r32 = 0 / 1) and the four-wave one (ng = 4), forward_batches, forward_small,
forward_gather (E rows bit-exact), the per-layer bf16 forward, the one-launch bf16 forward unfolded / folded / as a
batch set, the int8 forward and its batch set, the MLP-free model lone and as a set at p3ng = 4 / 8 -- with the serving
copy off, f32, fp16 and int8 wherever test_gpu_half_tables / test_gpu_int8_tables compose the two; serving_copy_bytes,
the source table after packing, index n and -1 on the huge field.  G2 (8.6 GB table): forward on eight and four waves,
forward_gather, forward_batches, copy on and off.  G1-QR (mult, add): forward on both kernels and forward_gather.
Training through the C ABI on G1, both G1-QR variants and G2, the same cases on each: dfwfm_train_forward (with helper
waves where the shape has them, and ftrain = 0), dfwfm_backward sorted on both batches and atomic on once, TILES then
SPREAD beside MLP_WEIGHTS, the four phases singly, dfwfm_backward_phases_bce, dropout 0 and 0.5.  The touched-row lists
on G1 and both G1-QR variants, with the huge table first in `dest` (every later table past 2^30 floats) and the stamps
preset to 0x7fffffff.  Optimizers at weight_decay 0: dfwfm_lazy_adam_step_dev and dfwfm_lazy_optim_step_dev (sgd,
momentum, adag, rmsp) on G1 and both G1-QR variants, two steps; plain lazy SGD and dfwfm_optim_step (one tensor of
2,147,484,800 floats against dfwfm_optim_elem_ref) on G2; FusedTrainStep on G1 with lazy Adam, lazy SGD and dense SGD,
three steps and a step_many of two, then the refreshed serving copy.

Left out on G2, for the 24 GB cap on this module's device memory: the lazy steps that carry state (table + gradient +
state = 25.8 GB) and the touched-row lists (table + flat + local + stamps = 35 GB).  Not crossed by these geometries
and not claimed: the int8 copy of G1 (16 B per row: 1.7 GB), byte 2^31 of a first-order table (2^29 rows), and an
`int` element product in a kernel that only G1 reaches (big_table_cases: what each geometry can witness).

The geometries share the device one at a time: the tests are written to run in file order, and a geometry's fixture
closes the one before it (a test that then still holds a closed geometry gets a RuntimeError saying so)."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import big_table_cases as bt
import optim_ref
from test_gpu_exact_train import Abi
from test_gpu_parity import make_model
from test_gpu_tables import _set, _small, dev

pytestmark = pytest.mark.gpu

GB = 10 ** 9
CAP = 24 * GB  # device memory this module may hold at once; a geometry is built when CAP + HEADROOM is free
HEADROOM = 8 * GB
POISON = bt.POISON
_LIVE = []


# ------------------------------------------------------------------------------------------------ huge model and twin
class Pair:
    """The huge model and its twin on the device, for one geometry; deep and MLP-free, the latter on the same
    Parameters.  Never materialises a huge array on the host."""

    def __init__(self, name, gpu):
        self.name, self.gpu, self.geo = name, gpu, bt.GEOS[name]
        free, total = torch.cuda.mem_get_info()
        if free < CAP + HEADROOM:
            pytest.skip(f"{name}: needs {CAP} + {HEADROOM} bytes of free device memory, {free} of {total} are free")
        torch.cuda.reset_peak_memory_stats()
        self.cfg, self.params = bt.twin(name)
        self.idx = torch.from_numpy(self.geo.probed).to(gpu)
        self.names = bt.table_names(self.geo)
        self.twin = make_model(self.cfg, self.params, gpu)
        self.huge = make_model(self.cfg, self.params, gpu)
        for k in self.names:
            mod, attr = self._owner(self.huge, k)
            small = getattr(mod, attr).detach()
            big = torch.empty(self.geo.rows, small.shape[1], device=gpu).fill_(POISON)
            big[self.idx] = small
            setattr(mod, attr, torch.nn.Parameter(big))
            if self.geo.qr:
                mod.num_categories = self.geo.keys
        scfg, sparams = bt.shallow(self.cfg, self.params)
        self.twin_shallow = make_model(scfg, sparams, gpu)
        self.huge_shallow = make_model(scfg, sparams, gpu)
        for k in self.names:  # the same tables, not a second 4 GB
            mod, attr = self._owner(self.huge_shallow, k)
            setattr(mod, attr, dict(self.huge.named_parameters())[k])
            if self.geo.qr:
                mod.num_categories = self.geo.keys
        self.peak = 0

    @staticmethod
    def _owner(m, name):
        fam, f, attr = name.split(".")
        return getattr(m, fam)[int(f)], attr

    def models(self):
        return (self.huge, self.twin, self.huge_shallow, self.twin_shallow)

    def fresh(self):
        """New engines (DFWFM_DIAG's r32 and ng are read when a model is created; the serving copy's allocation only
        grows) and the default switches; whatever a test cached on the old engines goes with them."""
        for k in ("_abis", "_abis_local", "_stamp"):
            self.__dict__.pop(k, None)
        # the peak since the last call: torch's tensors plus the library's serving copies that were alive with them
        copies = sum(m._engine.serving_copy_bytes() for m in self.models()
                     if m._engine is not None and m._engine.handle is not None)
        self.peak = max(self.peak, torch.cuda.max_memory_allocated() + copies)
        assert self.peak <= CAP, f"{self.name}: {self.peak} bytes of device memory at once, the cap is {CAP}"
        for m in self.models():
            if m._engine is not None:
                m._engine.close()
                m._engine = None
            m.pack_tables, m.table_dtype, m.mlp_dtype, m.bf16_fused, m.bf16_fold = True, "f32", "f32", False, False
            m.small_batch_rows, m.strict_index_check = 0, True
            m.eval()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    def table(self, k):
        return dict(self.huge.named_parameters())[k]

    def restore(self):
        """The parameters as built: after a test that trained them."""
        with torch.no_grad():
            for m in (self.huge, self.twin):
                for k, p in m.named_parameters():
                    src = torch.from_numpy(self.params[k]).to(self.gpu)
                    if m is self.huge and k in self.names:
                        p.fill_(POISON)
                        p[self.idx] = src
                    else:
                        p.copy_(src)
                    p.grad = None

    def assert_tables_intact(self, what):
        """The huge tables still hold the twin's rows at the probed rows and POISON everywhere else."""
        for k in self.names:
            t = self.table(k).detach()
            assert torch.equal(t[self.idx], torch.from_numpy(self.params[k]).to(self.gpu)), (what, k)
            assert_complement(t, self.idx, POISON, (what, k))

    def close(self):
        self.fresh()
        print(f"\n[big tables] {self.name}: peak device memory {self.peak / GB:.2f} GB (tensors and serving copies)")
        name = self.name
        self.__dict__.clear()
        self.closed = name

    def __getattr__(self, k):  # (only reached for a missing attribute: everything is gone after close())
        closed = self.__dict__.get("closed")
        if closed:
            raise RuntimeError(f"the {closed} geometry was closed when the next one was built: this module's tests "
                               "run in file order, one geometry at a time")
        raise AttributeError(k)


def assert_complement(t, idx, value, what):
    """Every row of t outside idx is `value` (t's rows at idx are saved, overwritten for the check and put back)."""
    keep = t[idx].clone()
    t[idx] = value
    # reductions without a temporary of t's size; min / max propagate a NaN, which then equals nothing
    ok = bool(t.min() == value) and bool(t.max() == value) if value else not bool(t.any())
    t[idx] = keep
    assert ok, (what, "an element outside the probed rows changed")


def _release():
    while _LIVE:
        _LIVE.pop().close()
    gc.collect()
    torch.cuda.empty_cache()


def _geometry(name, gpu):
    _release()  # one geometry on the device at a time
    p = Pair(name, gpu)
    _LIVE.append(p)
    yield p
    _release()


@pytest.fixture(scope="module")
def g1(gpu):
    yield from _geometry("g1", gpu)


@pytest.fixture(scope="module")
def g1qr_mult(gpu):
    yield from _geometry("g1qr_mult", gpu)


@pytest.fixture(scope="module")
def g1qr_add(gpu):
    yield from _geometry("g1qr_add", gpu)


@pytest.fixture(scope="module")
def g2(gpu):
    yield from _geometry("g2", gpu)


# ------------------------------------------------------------------------------------------------ inference
def _module(m, xi, xv, gpu):
    with torch.no_grad():
        out = m(*dev(gpu, xi, xv))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _gather(m, xi, xv, gpu):
    with torch.no_grad():
        E, fs = m._sync_inference(gpu).forward_gather(*dev(gpu, xi, xv))
    m.check_index_errors()
    return np.concatenate([E.cpu().numpy(), fs.cpu().numpy()[:, None]], axis=1)


ALL, F32 = ("off", "f32", "fp16", "int8"), ("off", "f32")
FUSED = dict(mlp_dtype="bf16", bf16_fused=True)
# name: (MLP-free model, module switches, DFWFM_DIAG, forward, serving copies it composes with, engine state after)
ROUTES = {
    "f32_r32_0": (0, {}, "r32=0", _module, ALL, {}),
    "f32_r32_1": (0, {}, "r32=1", _module, ALL, {}),
    "f32_ng4": (0, {}, "ng=4", _module, ALL, {}),
    "batches": (0, {}, None, _set("forward_batches"), ALL, {}),
    "small": (0, dict(small_batch_rows=64), None, _small, F32, {}),
    "gather": (0, {}, None, _gather, F32, {}),
    "bf16": (0, dict(mlp_dtype="bf16"), None, _module, F32, dict(bf16=True, bf16_fused=False)),
    "bf16_fused": (0, FUSED, None, _module, ALL, dict(bf16_fused=True, _bf16_fold_on=False)),
    "bf16_fold": (0, dict(FUSED, bf16_fold=True), None, _module, ALL, dict(bf16_fused=True, _bf16_fold_on=True)),
    "bf16_set": (0, FUSED, None, _set("forward_bf16_batches"), ALL, dict(bf16_fused=True)),
    "int8": (0, dict(mlp_dtype="int8"), None, _module, ALL, dict(int8=True)),
    "int8_set": (0, dict(mlp_dtype="int8"), None, _set("forward_int8_batches"), ALL, dict(int8=True)),
    "shallow_p3ng4": (1, {}, "p3ng=4", _module, ALL, {}),
    "shallow_p3ng8": (1, {}, "p3ng=8", _module, ALL, {}),
    "shallow_set_p3ng4": (1, {}, "p3ng=4", _set("forward_batches"), ALL, {}),
    "shallow_set_p3ng8": (1, {}, "p3ng=8", _set("forward_batches"), ALL, {}),
}
ROW_BYTES = {"f32": 64, "fp16": 32, "int8": 16}
G1_CASES = [(r, c) for r, v in ROUTES.items() for c in v[4]]


def _run_route(pair, monkeypatch, route, copy, kinds=("dup", "dup_rev", "once")):
    shallow, switches, diag, fwd, copies, state = ROUTES[route]
    assert copy in copies
    if diag:
        monkeypatch.setenv("DFWFM_DIAG", diag)
    pair.fresh()
    huge, twin = (pair.huge_shallow, pair.twin_shallow) if shallow else (pair.huge, pair.twin)
    for m in (huge, twin):
        for k, v in switches.items():
            setattr(m, k, v)
        m.pack_tables, m.table_dtype = copy != "off", "f32" if copy == "off" else copy
    for kind in kinds:
        xi_h, xi_t, xv, _, _ = bt.batch(pair.name, kind)
        got, want = fwd(huge, xi_h, xv, pair.gpu), fwd(twin, xi_t, xv, pair.gpu)
        assert np.isfinite(want).all() and np.abs(want).max() < 100, (route, copy, kind)  # no POISON in the twin
        assert np.array_equal(got, want), (route, copy, kind, np.flatnonzero((got != want).reshape(len(got), -1).any(1)))
        for m in (huge, twin):
            on = copy != "off" and not pair.geo.qr  # (the copy does not cover a model with a QR field)
            assert m._engine._packed_on is on, (route, copy)
            for k, v in state.items():
                assert getattr(m._engine, k) is v, (route, k)
    return huge


@pytest.mark.parametrize("route,copy", G1_CASES)
def test_g1_inference(g1, monkeypatch, route, copy):
    huge = _run_route(g1, monkeypatch, route, copy)
    if copy != "off":  # the copy's size, and the source table after packing
        rows = sum(g1.cfg["feature_sizes"][bt.NUM:]) - g1.geo.K + g1.geo.rows
        assert huge._engine.serving_copy_bytes() == rows * ROW_BYTES[copy]
    if route in ("f32_r32_1", "shallow_p3ng8"):
        g1.assert_tables_intact((route, copy))


@pytest.mark.parametrize("copy", ALL)
@pytest.mark.parametrize("bad", ["n", "-1"])
def test_g1_index_range_on_the_huge_field(g1, bad, copy):
    """Index n1 and -1 on the huge field raise IndexError through the flag, and the kernel read row 0 for them."""
    g1.fresh()
    xi_h, xi_t, xv, _, _ = bt.batch("g1", "dup")
    xi_h, xi_t = xi_h.copy(), xi_t.copy()
    xi_h[9, bt.FIELD] = g1.geo.rows if bad == "n" else -1
    xi_t[9, bt.FIELD] = 0
    for m in (g1.huge, g1.twin):
        m.pack_tables, m.table_dtype = copy != "off", "f32" if copy == "off" else copy
    with pytest.raises(IndexError):
        _module(g1.huge, xi_h, xv, g1.gpu)
    g1.huge.strict_index_check = False
    got = _module(g1.huge, xi_h, xv, g1.gpu)
    assert g1.huge._engine.read_error_flag() != 0
    assert np.array_equal(got, _module(g1.twin, xi_t, xv, g1.gpu))


# ------------------------------------------------------------------------------------------------ the training step
class BigAbi(Abi):
    """test_gpu_exact_train.Abi with the huge field's tables FIRST in the flat gradient buffer (every later table's
    offset is past them), and both gradient descriptors on one object: dense (every table in `flat`) and local (the
    categorical tables in `local`, for the touched-row lists)."""

    def __init__(self, m, gpu, first, local=False):
        from xsdeepfwfm_deprecated_amd import _lib
        self.m, self.gpu, self.lib, self.L = m, gpu, _lib, _lib.lib()
        self.eng = m._sync_engine(gpu)
        self.fields, self.dense = m._param_layout()
        named = dict(m.named_parameters())
        params = [named[k] for k in first] + [p for k, p in named.items() if k not in first and p.requires_grad]
        self.flat = torch.zeros(sum(p.numel() for p in params), device=gpu)
        self.local = torch.zeros_like(self.flat) if local else None
        self.off, off = {}, 0
        for p in params:
            self.off[id(p)] = off
            off += p.numel()
        self.names = {id(p): k for k, p in named.items()}
        self.shapes = {id(p): tuple(p.shape) for p in params}
        H = len(self.dense["lin_w"])
        d = self.dense
        self._keep = []

        def grads(cat_base):
            fb = self.flat.data_ptr()
            ptr = lambda t, f=-1: None if t is None else (cat_base if f >= m.num else fb) + 4 * self.off[id(t)]  # noqa
            fg = (_lib.dfwfm_field_grads * len(self.fields))(
                *[_lib.dfwfm_field_grads(*[ptr(t, f) for t in tup]) for f, tup in enumerate(self.fields)])
            gW = (ctypes.c_void_p * max(H, 1))(*[ptr(t) for t in d["lin_w"]])
            gB = (ctypes.c_void_p * max(H, 1))(*[ptr(t) for t in d["lin_b"]])
            self._keep += [fg, gW, gB]
            return _lib.dfwfm_grads(fg, ptr(d["field_cov"]), ptr(d["fwfm_lin"]), ptr(d["fm_1st"]), ptr(d["bias"]),
                                    gW if H else None, gB if H else None, ptr(d["fc_w"]))
        self.grads_dense = grads(self.flat.data_ptr())
        self.grads_local = grads(self.local.data_ptr()) if local else None
        self.grads = self.grads_dense

    def forward_on(self, xi, xv, dl, drop_p, seed):
        self.xi, self.xv, self.dl = dev(self.gpu, xi, xv, dl)
        self.out = torch.empty(len(xi), device=self.gpu)
        self.eng.train_forward(self.xi, self.xv, self.out, drop_p, seed)
        return self.out


SEED = 20261
TRAIN_ROUTES = ("whole", "tiles-spread", "single", "bce")


def _abis(pair, local=False):
    """One BigAbi per model, kept for the geometry (their flat buffers are zeroed before every use)."""
    key = "_abis_local" if local else "_abis"
    if key not in pair.__dict__:
        pair.fresh()
        gc.collect()
        torch.cuda.empty_cache()
        pair.__dict__[key] = tuple(BigAbi(m, pair.gpu, pair.names, local) for m in (pair.huge, pair.twin))
    return pair.__dict__[key]


def _backward(a, route, y, B):
    if route != "bce":
        a.backward(route)
        return None
    loss = torch.zeros(1, device=a.gpu)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dl = torch.full((B,), 7.0, device=a.gpu)
    a.lib.check(a.L.dfwfm_backward_phases_bce(a.eng.handle, p(a.out), p(y), float(B), p(dl), p(loss),
                                              ctypes.byref(a.grads), a.lib.BWD_TABLES | a.lib.BWD_MLP_WEIGHTS,
                                              a.stream()), "bwd bce")
    torch.cuda.synchronize()
    return torch.cat([dl, loss]).cpu().numpy()


def _compare_flat(pair, ah, at, what, huge_only=False):
    """The huge model's flat gradient buffer against the twin's: the probed rows of the huge tables and (unless
    huge_only) every other parameter, bit for bit; then, with all of those zeroed, nothing else in the buffer."""
    torch.cuda.synchronize()
    K = pair.geo.K
    for i, o in at.off.items():
        k = at.names[i]
        n = int(np.prod(at.shapes[i]))
        want = at.flat[o:o + n]
        oh = ah.off[id(dict(ah.m.named_parameters())[k])]
        if k in pair.names:
            w = n // K
            view = ah.flat[oh:oh + pair.geo.rows * w].view(pair.geo.rows, w)
            assert want.any(), (what, k, "the twin's gradient is zero: nothing compared")
            assert torch.equal(view[pair.idx], want.view(K, w)), (what, k)
            view[pair.idx] = 0.0
        else:
            assert huge_only or torch.equal(ah.flat[oh:oh + n], want), (what, k)
            ah.flat[oh:oh + n] = 0.0
    assert not bool(ah.flat.any()), (what, "a gradient outside the probed rows")


def _train_case(pair, monkeypatch, route, kind, det, drop, ftrain="1"):
    monkeypatch.setenv("DFWFM_DIAG", f"ftrain={ftrain}")
    xi_h, xi_t, xv, y, dl = bt.batch(pair.name, kind)
    ah, at = _abis(pair)
    extra = []
    for a, xi in ((ah, xi_h), (at, xi_t)):
        a.flat.zero_()
        a.eng.set_deterministic(det)
        a.forward_on(xi, xv, dl, 0.5 if drop else 0.0, SEED)
        extra.append(_backward(a, route, dev(a.gpu, y)[0], len(xi)))
    what = (pair.name, route, kind, det, drop, ftrain)
    assert torch.equal(ah.out, at.out) and bool(torch.isfinite(at.out).all()), (what, "logits")
    if route == "bce":
        assert np.array_equal(*extra), (what, "dlogit and loss")
    _compare_flat(pair, ah, at, what, huge_only=not det)


def _train_params(geos):
    out = []
    for name in geos:
        for route in TRAIN_ROUTES:
            for drop in (False, True):
                out += [(name, route, "dup", True, drop), (name, route, "once", True, drop),
                        (name, route, "once", False, drop)]
    return out


@pytest.mark.parametrize("route,kind,det,drop", [c[1:] for c in _train_params(["g1"])],
                         ids=lambda v: {True: "y", False: "n"}.get(v, v))
def test_g1_training_step(g1, monkeypatch, route, kind, det, drop):
    _train_case(g1, monkeypatch, route, kind, det, drop)


@pytest.mark.parametrize("kind", ["dup", "once"])
def test_g1_training_forward_without_helper_waves(g1, monkeypatch, kind):
    _train_case(g1, monkeypatch, "whole", kind, True, True, ftrain="0")


def _map_dest(pair, d):
    """A twin list destination as the huge model's: both layouts have the huge field's tables first."""
    K, n, D = pair.geo.K, pair.geo.rows, pair.geo.D
    d = np.asarray(d, np.int64)
    row2 = pair.geo.probed[np.minimum(d // D, K - 1)] * D + d % D
    row1 = n * D + pair.geo.probed[np.clip(d - K * D, 0, K - 1)]
    return np.where(d < K * D, row2, np.where(d < K * (D + 1), row1, d - K * (D + 1) + n * (D + 1)))


def _lists(a, B, stamp):
    """test_gpu_exact_train._lists_step's plumbing after a backward into the local buffer; returns per family the
    (dest, rows) of the list sorted by destination."""
    lib, L, m = a.lib, a.L, a.m
    out = []
    for fam, (iq, ir) in ((0, (0, 1)), (1, (2, 3))):
        o = lambda t: -1 if t is None else a.off[id(t)]  # noqa: E731
        dest = (lib.dfwfm_sparse_dest * len(a.fields))(
            *[lib.dfwfm_sparse_dest(o(tup[iq]) if f >= m.num else -1, o(tup[ir]) if f >= m.num else -1)
              for f, tup in enumerate(a.fields)])
        cap, w, wsb = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        lib.check(L.dfwfm_sparse_grads_size(a.eng.handle, fam, B, ctypes.byref(cap), ctypes.byref(w),
                                            ctypes.byref(wsb)), "size")
        od = torch.full((cap.value,), -7, dtype=torch.int64, device=a.gpu)
        orow = torch.zeros(cap.value * w.value, device=a.gpu)
        cnt = torch.zeros(1, dtype=torch.int32, device=a.gpu)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        lib.check(L.dfwfm_sparse_grads_local(a.eng.handle, fam, dest, cap.value, p(a.local), p(stamp), a.local.numel(),
                                             p(od), p(orow), p(cnt), a.stream()), "local lists")
        lib.check(L.dfwfm_sparse_grads_apply(p(a.flat), w.value, p(od), p(orow), p(cnt), cap.value, a.stream()),
                  "apply")
        torch.cuda.synchronize()
        n = int(cnt.item())
        assert 0 < n <= cap.value
        d = od[:n].cpu().numpy()
        order = np.argsort(d)
        assert len(np.unique(d)) == n
        out.append((d[order], orow.view(cap.value, w.value)[:n].cpu().numpy()[order]))
    return out


def _lists_case(pair, kind, det):
    """The touched-row lists of both families: the destinations are the twin's under the map, the rows equal bit for
    bit (sorted route; atomic on `once`: the huge field's entries), the local buffer is zero again, and apply into the
    zero flat buffer gives the dense gradient -- compared with the twin's like every backward's."""
    xi_h, xi_t, xv, y, dl = bt.batch(pair.name, kind)
    ah, at = _abis(pair, local=True)
    if "_stamp" not in pair.__dict__:
        pair._stamp = [torch.empty(a.flat.numel() + 1, dtype=torch.int32, device=pair.gpu) for a in (ah, at)]
    res = []
    for a, xi, stamp in ((ah, xi_h, pair._stamp[0]), (at, xi_t, pair._stamp[1])):
        stamp.fill_(0x7fffffff)
        a.flat.zero_()
        a.grads = a.grads_local
        a.eng.set_deterministic(det)
        a.forward_on(xi, xv, dl, 0.0, 0)
        a.backward("whole")
        a.grads = a.grads_dense
        res.append(_lists(a, len(xi), stamp))
        assert not bool(a.local.any()), "local buffer not zero"
    first = pair.geo.rows * (pair.geo.D + 1)
    for (dh, rh), (dt, rt) in zip(*res):
        want = _map_dest(pair, dt)
        assert np.all(np.diff(want) > 0)  # the map is monotone: the sorted orders correspond
        assert np.array_equal(dh, want)
        keep = slice(None) if det else dh < first
        assert np.array_equal(rh[keep], rt[keep]) and (dh < first).sum() == pair.geo.K
    _compare_flat(pair, ah, at, (pair.name, "lists", kind, det), huge_only=not det)


@pytest.mark.parametrize("kind,det", [("dup", True), ("once", True), ("once", False)], ids=["dup", "once", "once-atomic"])
def test_g1_touched_row_lists(g1, kind, det):
    _lists_case(g1, kind, det)


# ------------------------------------------------------------------------------------------------ optimizers
LAZY = [("adam", 0.0), ("sgd", 0.0), ("sgd", 0.9), ("adag", 0.0), ("rmsp", 0.0)]
LAZY_IDS = ["adam", "sgd", "sgd-momentum", "adag", "rmsp"]


def _lazy_tables(pair, m, n_state, rows_of):
    """The huge field's tables of model m as lazy-step tables: p the Parameter itself, g / state fresh (g random on the
    probed rows, the same values for both models), one stamp per row."""
    from xsdeepfwfm_deprecated_amd import _lib
    named = dict(m.named_parameters())
    geo, out = pair.geo, []
    r = np.random.default_rng(77)
    keys = list(pair.names) + ([k.replace("weight_q", "weight_r") for k in pair.names] if geo.qr else [])
    for k in keys:
        p = named[k].detach()
        rem = k.endswith("weight_r")
        rows, width = p.shape
        src = (r.standard_normal((rows if rem else geo.K, width)) * 0.1).astype(np.float32)
        g = torch.zeros_like(p)
        g[slice(None) if rem or rows == geo.K else pair.idx] = torch.from_numpy(src).to(pair.gpu)
        kind = _lib.LAZY_REMAINDER if rem else (_lib.LAZY_QUOTIENT if geo.qr else _lib.LAZY_PLAIN)
        out.append(dict(name=k, p=p, g=g, s=[torch.zeros_like(p) for _ in range(n_state)],
                        stamp=torch.zeros(rows, dtype=torch.int32, device=pair.gpu), rows=rows, width=width,
                        key_range=rows_of(m), c=geo.c, kind=kind, huge=rows == geo.rows))
    return out


def _lazy_step(opt, mom, tabs, xi, state, gpu):
    from xsdeepfwfm_deprecated_amd import _lib
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    x, ptr = ctypes.c_void_p(xi.data_ptr()), (lambda t: t.data_ptr())
    if opt == "adam":
        arr = (_lib.dfwfm_lazy_adam_table * len(tabs))(*[_lib.dfwfm_lazy_adam_table(
            ptr(t["p"]), ptr(t["g"]), ptr(t["s"][0]), ptr(t["s"][1]), ptr(t["stamp"]), t["rows"], t["key_range"],
            t["c"], t["width"], bt.FIELD, t["kind"], 0) for t in tabs])
        _lib.check(_lib.lib().dfwfm_lazy_adam_step_dev(arr, len(tabs), x, xi.stride(0), xi.shape[0], 1e-3, 0.9, 0.999,
                                                       1e-8, 0.0, ctypes.c_void_p(state.data_ptr()), st), "lazy adam")
        return
    arr = (_lib.dfwfm_lazy_optim_table * len(tabs))(*[_lib.dfwfm_lazy_optim_table(
        ptr(t["p"]), ptr(t["g"]), ptr(t["s"][0]) if t["s"] else None, ptr(t["stamp"]), t["rows"], t["key_range"],
        t["c"], t["width"], bt.FIELD, t["kind"], 0) for t in tabs])
    h = optim_ref.hyper(opt, 1e-2, 0.0, mom)
    _lib.check(_lib.lib().dfwfm_lazy_optim_step_dev(arr, len(tabs), x, xi.stride(0), xi.shape[0], ctypes.byref(h),
                                                    ctypes.c_void_p(state.data_ptr()), st), "lazy optim")


def _lazy_case(pair, opt, mom):
    """Two lazy steps (dup, then once with fresh gradients) on the huge field's tables of both models: parameters and
    state of the probed rows equal the twin's, gradients are zero again, and nothing outside the probed rows moved."""
    from xsdeepfwfm_deprecated_amd import _lib
    pair.fresh()
    gc.collect()
    torch.cuda.empty_cache()
    n_state = 2 if opt == "adam" else int(optim_ref.has_state(opt, mom))
    try:
        th = _lazy_tables(pair, pair.huge, n_state, lambda m: pair.geo.keys)
        tt = _lazy_tables(pair, pair.twin, n_state, lambda m: pair.geo.twin_keys)
        states = [torch.zeros(_lib.ADAM_STATE_BYTES // 8, dtype=torch.int64, device=pair.gpu) for _ in range(2)]
        for step, kind in enumerate(("dup", "once")):
            xi_h, xi_t, _, _, _ = bt.batch(pair.name, kind)
            if step:
                for a, b in zip(th, tt):  # fresh gradients: the twin's rows copied to the probed rows
                    b["g"].copy_(torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(b["g"].shape))
                                                  .astype(np.float32)).to(pair.gpu))
                    a["g"][pair.idx if a["huge"] else slice(None)] = b["g"]
            _lazy_step(opt, mom, th, dev(pair.gpu, xi_h)[0], states[0], pair.gpu)
            _lazy_step(opt, mom, tt, dev(pair.gpu, xi_t)[0], states[1], pair.gpu)
            torch.cuda.synchronize()
            assert torch.equal(*states)
            for a, b in zip(th, tt):
                what = (pair.name, opt, mom, step, a["name"])
                sel = pair.idx if a["huge"] else slice(None)
                assert not torch.equal(b["p"], torch.from_numpy(pair.params[a["name"]]).to(pair.gpu)), what
                assert torch.equal(a["p"][sel], b["p"]), what
                assert not bool(a["g"].any()) and not bool(b["g"].any()), what
                for sa, sb in zip(a["s"], b["s"]):
                    assert torch.equal(sa[sel], sb) and bool(sb.any()), what
                    if a["huge"]:
                        assert_complement(sa, pair.idx, 0.0, what)
                if a["huge"]:
                    assert_complement(a["p"], pair.idx, POISON, what)
    finally:
        th = tt = None
        pair.restore()


@pytest.mark.parametrize("opt,mom", LAZY, ids=LAZY_IDS)
def test_g1_lazy_optimizers(g1, opt, mom):
    _lazy_case(g1, opt, mom)


@pytest.mark.parametrize("mode", ["lazy_adam", "lazy_sgd", "dense_sgd"])
def test_g1_fused_train_step(g1, mode):
    """FusedTrainStep on both models, deterministic: an eager step, two replayed ones and a step_many of two.  Logits
    after every step, every parameter and moment equal the twin trainer's; the complement is untouched; and the next
    inference forward reads a refreshed serving copy (lazy Adam: the fp16 copy, for the 24 GB cap)."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    pair = g1
    pair.fresh()
    gc.collect()
    torch.cuda.empty_cache()
    kw = dict(lazy_adam=dict(lr=1e-3, lazy_table_adam=True), lazy_sgd=dict(lr=0.05, optimizer="sgd", lazy_tables=True),
              dense_sgd=dict(lr=0.05, optimizer="sgd"))[mode]
    copy = "fp16" if mode == "lazy_adam" else "f32"
    batches = [bt.batch("g1", k) for k in ("dup", "dup_rev", "dup", "dup_rev", "dup")]
    trainers, outs = [], []
    try:
        for m, col in ((pair.huge, 0), (pair.twin, 1)):
            m.is_deep_dropout = False
            m.table_dtype = copy
            xi0 = batches[0]
            before = _module(m, xi0[col], xi0[2], pair.gpu)  # packs the copy the steps must invalidate
            m.train()
            torch.manual_seed(5)
            t = FusedTrainStep(m, bt.B_DUP, weight_decay=0.0, deterministic=True, resident_inputs=True, **kw)
            trainers.append(t)
            devb = [dev(pair.gpu, b[col], b[2], b[3]) for b in batches]
            log = []
            for b in devb[:3]:
                t.step(*b)
                log.append(t.out.clone())
            t.step_many(devb[3:])
            log.append(t.out.clone())
            torch.cuda.synchronize()
            t.close()
            m.eval()
            after = _module(m, xi0[col], xi0[2], pair.gpu)
            assert m._engine._packed_on and not np.array_equal(after, before)
            outs.append((log, after))
        th, tt = trainers
        for a, b in zip(*[o[0] for o in outs]):
            assert torch.equal(a, b), (mode, "logits of a step")
        assert np.array_equal(outs[0][1], outs[1][1]), (mode, "inference after training")
        assert [pair_name(th, p) for p in th.params] == [pair_name(tt, p) for p in tt.params]
        for ph, pt, oh, ot in zip(th.params, tt.params, th.offs, tt.offs):
            k = pair_name(tt, pt)
            big = k in pair.names
            sel = pair.idx if big else slice(None)
            assert torch.equal(ph.detach()[sel], pt.detach()), (mode, k)
            if big:
                assert not torch.equal(pt.detach().cpu(), torch.from_numpy(pair.params[k])), (mode, k, "did not train")
                assert_complement(ph.detach(), pair.idx, POISON, (mode, k))
            for bh, btw in ((th.exp_avg, tt.exp_avg), (th.exp_avg_sq, tt.exp_avg_sq), (th.opt_state, tt.opt_state)):
                if bh is None:
                    continue
                sh, st_ = bh[oh:oh + ph.numel()].view_as(ph), btw[ot:ot + pt.numel()].view_as(pt)
                assert torch.equal(sh[sel], st_), (mode, k, "moment")
                if big:
                    assert_complement(sh, pair.idx, 0.0, (mode, k, "moment"))
    finally:
        trainers.clear()
        th = tt = t = None
        gc.collect()
        pair.restore()
        pair.fresh()


def pair_name(t, p):
    return next(k for k, q in t.model.named_parameters() if q is p)


# ------------------------------------------------------------------------------------------------ G1-QR
QR_ROUTES = ("f32_r32_0", "f32_r32_1", "gather")
STEP_CASES = [c[1:] for c in _train_params(["x"])]
STEP_IDS = lambda v: {True: "y", False: "n"}.get(v, v)  # noqa: E731
LIST_CASES = dict(argvalues=[("dup", True), ("once", True), ("once", False)], ids=["dup", "once", "once-atomic"])


@pytest.mark.parametrize("route", QR_ROUTES)
def test_g1qr_mult_inference(g1qr_mult, monkeypatch, route):
    _run_route(g1qr_mult, monkeypatch, route, "f32", kinds=("dup", "once"))


@pytest.mark.parametrize("route,kind,det,drop", STEP_CASES, ids=STEP_IDS)
def test_g1qr_mult_training_step(g1qr_mult, monkeypatch, route, kind, det, drop):
    _train_case(g1qr_mult, monkeypatch, route, kind, det, drop)


@pytest.mark.parametrize("kind", ["dup", "once"])
def test_g1qr_mult_training_forward_without_helper_waves(g1qr_mult, monkeypatch, kind):
    _train_case(g1qr_mult, monkeypatch, "whole", kind, True, True, ftrain="0")


@pytest.mark.parametrize("kind,det", **LIST_CASES)
def test_g1qr_mult_touched_row_lists(g1qr_mult, kind, det):
    _lists_case(g1qr_mult, kind, det)


@pytest.mark.parametrize("opt,mom", LAZY, ids=LAZY_IDS)
def test_g1qr_mult_lazy_optimizers(g1qr_mult, opt, mom):
    _lazy_case(g1qr_mult, opt, mom)


@pytest.mark.parametrize("route", QR_ROUTES)
def test_g1qr_add_inference(g1qr_add, monkeypatch, route):
    _run_route(g1qr_add, monkeypatch, route, "f32", kinds=("dup", "once"))


@pytest.mark.parametrize("route,kind,det,drop", STEP_CASES, ids=STEP_IDS)
def test_g1qr_add_training_step(g1qr_add, monkeypatch, route, kind, det, drop):
    _train_case(g1qr_add, monkeypatch, route, kind, det, drop)


@pytest.mark.parametrize("kind", ["dup", "once"])
def test_g1qr_add_training_forward_without_helper_waves(g1qr_add, monkeypatch, kind):
    _train_case(g1qr_add, monkeypatch, "whole", kind, True, True, ftrain="0")


@pytest.mark.parametrize("kind,det", **LIST_CASES)
def test_g1qr_add_touched_row_lists(g1qr_add, kind, det):
    _lists_case(g1qr_add, kind, det)


@pytest.mark.parametrize("opt,mom", LAZY, ids=LAZY_IDS)
def test_g1qr_add_lazy_optimizers(g1qr_add, opt, mom):
    _lazy_case(g1qr_add, opt, mom)


# ------------------------------------------------------------------------------------------------ G2
@pytest.mark.parametrize("copy", F32)
@pytest.mark.parametrize("route", ["f32_r32_0", "f32_ng4", "gather", "batches"])
def test_g2_inference(g2, monkeypatch, route, copy):
    """D = 32: the generic K loop on eight and on four waves (fwd32_kernel does not take the shape); element offsets
    past 2^31 in the table, byte offsets past 2^33."""
    _run_route(g2, monkeypatch, route, copy)
    if route == "batches":
        g2.assert_tables_intact((route, copy))


@pytest.mark.parametrize("route,kind,det,drop", STEP_CASES, ids=STEP_IDS)
def test_g2_training_step(g2, monkeypatch, route, kind, det, drop):
    """The training forward and the backward at D = 32: the scatter's row * w runs past 2^31 floats in the table's
    gradient (8.86 GB of tables and 8.86 GB of gradients)."""
    _train_case(g2, monkeypatch, route, kind, det, drop)


@pytest.mark.parametrize("kind", ["dup", "once"])
def test_g2_training_forward_with_ftrain_0(g2, monkeypatch, kind):
    _train_case(g2, monkeypatch, "whole", kind, True, True, ftrain="0")


def test_g2_lazy_sgd(g2):
    _lazy_case(g2, "sgd", 0.0)


def test_g2_dense_sgd_on_one_tensor_past_2_31_floats(g2):
    """dfwfm_optim_step, plain SGD, on the huge table and a gradient buffer of its size: numel 2,147,484,800, one
    tensor.  The probed rows against dfwfm_optim_elem_ref; with weight_decay 0 and a zero gradient every other element
    must keep POISON's bits."""
    from xsdeepfwfm_deprecated_amd import _lib
    pair = g2
    pair.fresh()
    gc.collect()
    torch.cuda.empty_cache()
    p = pair.table(pair.names[0]).detach()
    assert p.numel() == 2_147_484_800 > 2 ** 31
    gh = (np.random.default_rng(9).standard_normal((pair.geo.K, pair.geo.D)) * 0.1).astype(np.float32)
    g = torch.zeros_like(p)
    try:
        g[pair.idx] = torch.from_numpy(gh).to(pair.gpu)
        h = optim_ref.hyper("sgd", 1e-2, 0.0, 0.0)
        arr = (_lib.dfwfm_optim_tensor * 1)(_lib.dfwfm_optim_tensor(p.data_ptr(), g.data_ptr(), None, p.numel()))
        st = ctypes.c_void_p(torch.cuda.current_stream(pair.gpu).cuda_stream)
        _lib.check(_lib.lib().dfwfm_optim_step(arr, 1, ctypes.byref(h), 1, st), "dfwfm_optim_step")
        torch.cuda.synchronize()
        want, _ = optim_ref.lib_step(h, 1, pair.params[pair.names[0]], gh)
        assert not np.array_equal(want, pair.params[pair.names[0]])
        assert optim_ref.same_bits(p[pair.idx].cpu().numpy(), want)
        assert_complement(p, pair.idx, POISON, "dfwfm_optim_step")
        assert torch.equal(g[pair.idx].cpu(), torch.from_numpy(gh))  # the dense step leaves the gradient
    finally:
        g = None
        pair.restore()
