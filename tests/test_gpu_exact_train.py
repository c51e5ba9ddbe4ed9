"""GPU: every route of the HIP training step, bit for bit against the float64 reference, on the exact-arithmetic
cases of tests/exact_train_cases.py (the CPU leg, tests/test_exact_train_cases.py, shows that the cases carry the
certificate, that float32 arithmetic alone returns the reference's bits, and that the host kernels do).

Every assertion is np.array_equal against ref64 cast to float32 -- the logits and every element of every gradient
tensor, the exact zeros of the rows a batch did not touch included.  The cases make every product and partial sum a
float32 in any order, so the atomic routes are held to the same bits as the sorted ones, and a dropped, duplicated or
misplaced term of any size fails.

Routes.  Base model (Criteo-39: FwFM + deep + lw, 13 numerical fields, D 10, 3 x 400) at B = 1, 16, 17, 129, dropout
0 and 0.5 (masks: oracle/torch_port.dropout_masks), deterministic on and off: autograd (m(xi, xv); out.backward(dl)),
and the C ABI whole (dfwfm_train_forward + dfwfm_backward), TABLES then MLP_WEIGHTS, TILES then SPREAD beside
MLP_WEIGHTS on a second stream, and TILES, REDUCE, SCATTER, MLP_WEIGHTS singly; the touched-row lists (local buffer,
dfwfm_sparse_grads_local for both families, dfwfm_sparse_grads_apply, twice on one stamp array); accumulation (two
backwards into one buffer: exactly twice the reference); the training forward with helper waves and fwd_kernel<TRAIN>
(DFWFM_DIAG=ftrain=1 / 0).  The 4097-row case (2 x 64, D 4: a second pass of the sorted scatter holding one sample, a
field whose every sample hits one of 3 rows, a field with all-distinct rows) and eleven model variants at B = 37 through
autograd and the whole C ABI.  On the saturated case (every |z| >= 128, B = denom = 128): dfwfm_bce_grad then the
backward, dfwfm_backward_phases_bce whole and TILES then SPREAD, and FusedTrainStep with plain SGD -- eager and
capture steps at rate 0 leave every parameter bit-identical, one replayed step at 2^-6 gives p - 2^-6 g bit for bit --
deterministic on and off, lazy_tables, step_many; and the same with dropout 0.5 on, step k under the masks of
step_seed(t.seed, k - 1), rates 0, 0, 2^-6 on a device-resident schedule, step_many as two steps in one graph.

A record of one session on an MI355X (not reproducible from the tree): all cases passed as the kernels stood, the
file in 7 s.  A library built with three wrong-value slips put in on purpose -- dw_sum_kernel leaving out the last
split, sort_scatter_kernel without its second pass, one component of one sample's dE halved in scatter_kernel --
failed in that run the sorted 129-row cases (47 320 elements of net_1_linear_1.weight), the sorted 4097-row cases
(1 element of the hot row) and the atomic cases with more than 36 rows (1 element), and passed the rest."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import exact_train_cases as xc
from test_gpu_train import build

pytestmark = pytest.mark.gpu

DET = pytest.mark.parametrize("det", [True, False], ids=["sorted", "atomic"])
DROP = pytest.mark.parametrize("drop", [False, True], ids=["p0", "p0.5"])
ABI_ROUTES = ("whole", "tables-mlp", "tiles-spread", "single")


def _assert_bits(what, logits, grads, case, times=1):
    z, g = xc.ref32(case)
    if logits is not None:
        assert np.array_equal(logits, z), (what, "logits", np.flatnonzero(logits != z)[:8])
    assert set(grads) == set(g), what
    for k, r in g.items():
        got = grads[k]
        got = np.zeros_like(r) if got is None else got
        want = r * np.float32(times)
        assert got.shape == want.shape and np.array_equal(got, want), \
            (what, k, int(np.sum(got != want)), "elements differ, first at", np.argwhere(got != want)[:4].tolist())


def _writable(params):
    """Copies for torch.from_numpy (the cases' arrays are read-only)."""
    return {k: v.copy() for k, v in params.items()}


@functools.lru_cache(maxsize=None)
def _model(gpu, key):
    """One model per case family for the module; the routes read its parameters, none writes them."""
    case = _case(key, 129, False)
    return build(case.cfg, _writable(case.params), gpu, is_deep_dropout=True)


def _case(key, B, drop):
    if key == "base":
        return xc.base_case(B, drop)
    if key == "hot":
        return xc.hot_case()
    if key == "sat":
        return xc.saturated().case
    return xc.variant_case(key, drop)


def _dev(gpu, case):
    xi = torch.from_numpy(case.xi.copy()).to(gpu)
    xv = torch.from_numpy(case.xv.copy()).to(gpu)
    return xi, xv, torch.from_numpy(case.dlogit.copy()).to(gpu)


def _autograd(m, gpu, case, det):
    m.deterministic = det
    m.is_deep_dropout = case.masks is not None
    m.zero_grad(set_to_none=True)
    xi, xv, dl = _dev(gpu, case)
    torch.manual_seed(99)  # train_forward then draws case.seed (train_cases.dropout_seed)
    out = m(xi, xv)
    out.backward(dl)
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().cpu().numpy()) for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    return out.detach().cpu().numpy(), grads


class Abi:
    """The C ABI on a model: one flat zeroed gradient buffer laid out like the parameters (test_gpu_train._sparse_step's
    plumbing), optionally with the categorical tables' gradients in a second, local buffer at the same offsets."""

    def __init__(self, m, gpu, local=False):
        from xsdeepfwfm_deprecated_amd import _lib
        self.m, self.gpu, self.lib, self.L = m, gpu, _lib, _lib.lib()
        self.eng = m._sync_engine(gpu)
        self.fields, self.dense = m._param_layout()
        params = [p for p in m.parameters() if p.requires_grad]
        self.flat = torch.zeros(sum(p.numel() for p in params), device=gpu)
        self.local = torch.zeros_like(self.flat) if local else None
        self.off, off = {}, 0
        for p in params:
            self.off[id(p)] = off
            off += p.numel()
        self.names = {id(p): k for k, p in m.named_parameters()}
        self.shapes = {id(p): tuple(p.shape) for p in params}
        fb = self.flat.data_ptr()
        lb = self.local.data_ptr() if local else fb
        ptr = lambda t, f=-1: None if t is None else (lb if f >= m.num else fb) + 4 * self.off[id(t)]  # noqa: E731
        self.fg = (_lib.dfwfm_field_grads * len(self.fields))(
            *[_lib.dfwfm_field_grads(*[ptr(t, f) for t in tup]) for f, tup in enumerate(self.fields)])
        H = len(self.dense["lin_w"])
        self.gW = (ctypes.c_void_p * max(H, 1))(*[ptr(t) for t in self.dense["lin_w"]])
        self.gB = (ctypes.c_void_p * max(H, 1))(*[ptr(t) for t in self.dense["lin_b"]])
        d = self.dense
        self.grads = _lib.dfwfm_grads(self.fg, ptr(d["field_cov"]), ptr(d["fwfm_lin"]), ptr(d["fm_1st"]),
                                      ptr(d["bias"]), self.gW if H else None, self.gB if H else None, ptr(d["fc_w"]))

    def stream(self, s=None):
        return ctypes.c_void_p((s or torch.cuda.current_stream(self.gpu)).cuda_stream)

    def forward(self, case):
        self.xi, self.xv, self.dl = _dev(self.gpu, case)  # kept alive: the backward re-reads them
        self.out = torch.empty(len(case.xi), device=self.gpu)
        self.eng.train_forward(self.xi, self.xv, self.out, xc.drop_p(case), case.seed)
        return self.out

    def phases(self, bits, s=None, dl=None):
        dl = self.dl if dl is None else dl
        self.lib.check(self.L.dfwfm_backward_phases(self.eng.handle, ctypes.c_void_p(dl.data_ptr()),
                                                    ctypes.byref(self.grads), bits, self.stream(s)), "bwd phases")

    def backward(self, route, dl=None):
        lib = self.lib
        if route == "whole":
            dl = self.dl if dl is None else dl
            lib.check(self.L.dfwfm_backward(self.eng.handle, ctypes.c_void_p(dl.data_ptr()), ctypes.byref(self.grads),
                                            self.stream()), "bwd")
        elif route == "tables-mlp":
            self.phases(lib.BWD_TABLES, dl=dl)
            self.phases(lib.BWD_MLP_WEIGHTS, dl=dl)
        elif route == "tiles-spread":
            self.phases(lib.BWD_TILES, dl=dl)
            self.fork_spread(dl)
        elif route == "single":
            for bits in (lib.BWD_TILES, lib.BWD_REDUCE, lib.BWD_SCATTER, lib.BWD_MLP_WEIGHTS):
                self.phases(bits, dl=dl)
        else:
            raise AssertionError(route)

    def fork_spread(self, dl=None):
        """MLP_WEIGHTS on a second stream beside SPREAD (the one-GPU step's fork)."""
        cur = torch.cuda.current_stream(self.gpu)
        side = torch.cuda.Stream(self.gpu)
        side.wait_stream(cur)
        self.phases(self.lib.BWD_MLP_WEIGHTS, side, dl=dl)
        self.phases(self.lib.BWD_SPREAD, dl=dl)
        cur.wait_stream(side)

    def result(self, buf=None):
        torch.cuda.synchronize()
        host = (self.flat if buf is None else buf).cpu().numpy()
        return {self.names[i]: host[o:o + int(np.prod(self.shapes[i]))].reshape(self.shapes[i]).copy()
                for i, o in self.off.items()}


def _abi(m, gpu, case, route, det, times=1):
    a = Abi(m, gpu)
    a.eng.set_deterministic(det)
    for _ in range(times):
        a.forward(case)
        a.backward(route)
    return a.out.cpu().numpy(), a.result()


# ------------------------------------------------------------------------------------------------- the base model
@DET
@DROP
@pytest.mark.parametrize("B", xc.BASE_B)
def test_base_autograd(gpu, B, drop, det):
    case = _case("base", B, drop)
    _assert_bits(f"autograd B={B}", *_autograd(_model(gpu, "base"), gpu, case, det), case)


@DET
@DROP
@pytest.mark.parametrize("B", xc.BASE_B)
@pytest.mark.parametrize("route", ABI_ROUTES)
def test_base_c_abi(gpu, route, B, drop, det):
    case = _case("base", B, drop)
    _assert_bits(f"{route} B={B}", *_abi(_model(gpu, "base"), gpu, case, route, det), case)


@DET
@pytest.mark.parametrize("route", ("whole", "tiles-spread"))
def test_base_backward_accumulates(gpu, route, det):
    """The backward adds into the gradient buffers: two steps into one buffer give exactly twice the reference."""
    case = _case("base", 129, True)
    _assert_bits(f"{route} twice", *_abi(_model(gpu, "base"), gpu, case, route, det, times=2), case, times=2)


def _lists_step(a, case, det, stamp):
    """Backward with the categorical tables scattered into the local buffer, then dfwfm_sparse_grads_local for both
    families and dfwfm_sparse_grads_apply into the (zero) flat buffer (test_gpu_train._local_lists_step's plumbing)."""
    lib, L, m = a.lib, a.L, a.m
    a.eng.set_deterministic(det)
    a.forward(case)
    a.backward("whole")
    n_lists = 0
    for fam, (iq, ir) in ((0, (0, 1)), (1, (2, 3))):
        o = lambda t: -1 if t is None else a.off[id(t)]  # noqa: E731
        dest = (lib.dfwfm_sparse_dest * len(a.fields))(
            *[lib.dfwfm_sparse_dest(o(tup[iq]) if f >= m.num else -1, o(tup[ir]) if f >= m.num else -1)
              for f, tup in enumerate(a.fields)])
        cap, w, wsb = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        lib.check(L.dfwfm_sparse_grads_size(a.eng.handle, fam, len(case.xi), ctypes.byref(cap), ctypes.byref(w),
                                            ctypes.byref(wsb)), "size")
        if cap.value == 0:
            continue
        od = torch.full((cap.value,), -7, dtype=torch.int64, device=a.gpu)
        orow = torch.zeros(cap.value * w.value, device=a.gpu)
        cnt = torch.zeros(1, dtype=torch.int32, device=a.gpu)
        lib.check(L.dfwfm_sparse_grads_local(a.eng.handle, fam, dest, cap.value, ctypes.c_void_p(a.local.data_ptr()),
                                             ctypes.c_void_p(stamp.data_ptr()), a.local.numel(),
                                             ctypes.c_void_p(od.data_ptr()), ctypes.c_void_p(orow.data_ptr()),
                                             ctypes.c_void_p(cnt.data_ptr()), a.stream()), "local lists")
        lib.check(L.dfwfm_sparse_grads_apply(ctypes.c_void_p(a.flat.data_ptr()), w.value,
                                             ctypes.c_void_p(od.data_ptr()), ctypes.c_void_p(orow.data_ptr()),
                                             ctypes.c_void_p(cnt.data_ptr()), cap.value, a.stream()), "apply")
        torch.cuda.synchronize()
        n = int(cnt.item())
        assert 0 < n <= cap.value and len(np.unique(od[:n].cpu().numpy())) == n  # one entry per touched row
        n_lists += 1
    return n_lists


@DET
@pytest.mark.parametrize("key,B,drop", [("base", 129, False), ("base", 129, True), ("base", 17, False),
                                        ("base", 17, True), ("hot", xc.HOT_B, False)],
                         ids=["base-129-p0", "base-129-p0.5", "base-17-p0", "base-17-p0.5", "hot"])
def test_touched_row_lists(gpu, key, B, drop, det):
    """The data-parallel step's list builder gives the tables' gradients back through apply, exactly, and leaves the
    local buffer exactly zero; twice on one stamp array."""
    case = _case(key, B, drop)
    a = Abi(_model(gpu, key), gpu, local=True)
    stamp = torch.zeros(a.flat.numel() + 1, dtype=torch.int32, device=gpu)
    for rep in range(2):
        a.flat.zero_()
        assert _lists_step(a, case, det, stamp) == 2  # both families
        assert not bool(a.local.any()), ("local buffer not zero", rep)
        _assert_bits(f"lists {key} rep {rep}", a.out.cpu().numpy(), a.result(), case)


@pytest.mark.parametrize("ft", ["0", "1"], ids=["fwd_kernel", "helper-waves"])
@DROP
@pytest.mark.parametrize("key,B", [("base", 17), ("base", 129), ("h1", xc.VARIANT_B)],
                         ids=["base-17", "base-129", "h1-37"])
def test_train_forward_variants(gpu, monkeypatch, key, B, drop, ft):
    """fwd_kernel<TRAIN> (DFWFM_DIAG=ftrain=0) and the helper-wave forward (ftrain_kernel), whose saved activations
    feed the backward: both give the reference's bits, sorted and atomic; on the base model and on the smallest shape
    the helper-wave forward takes (one hidden layer of 400)."""
    monkeypatch.setenv("DFWFM_DIAG", f"ftrain={ft}")
    case = _case(key, B, drop)
    for det in (True, False):
        _assert_bits(f"ftrain={ft} {key} B={B}", *_abi(_model(gpu, key), gpu, case, "whole", det), case)


# ------------------------------------------------------------------------------------------------- 4097 rows, variants
@DET
@pytest.mark.parametrize("route", ("autograd",) + ABI_ROUTES)
def test_hot_rows_4097(gpu, route, det):
    case = _case("hot", xc.HOT_B, False)
    m = _model(gpu, "hot")
    got = _autograd(m, gpu, case, det) if route == "autograd" else _abi(m, gpu, case, route, det)
    _assert_bits(f"hot {route}", *got, case)


@DET
@pytest.mark.parametrize("route", ("autograd", "whole"))
@pytest.mark.parametrize("name", list(xc.VARIANTS))
def test_model_variants(gpu, name, route, det):
    case = _case(name, xc.VARIANT_B, False)
    m = _model(gpu, name)
    got = _autograd(m, gpu, case, det) if route == "autograd" else _abi(m, gpu, case, route, det)
    _assert_bits(f"{name} {route}", *got, case)


# ------------------------------------------------------------------------------------------------- fused loss
def _assert_loss(what, dl, loss, sat):
    assert np.array_equal(dl, sat.case.dlogit), (what, "dlogit")
    assert loss == np.float32(sat.loss_sum) and float(np.float32(sat.loss_sum)) == sat.loss_sum, (what, loss)


@DET
@pytest.mark.parametrize("route", ("bce_grad", "bce-whole", "bce-tiles-spread"))
def test_saturated_fused_loss(gpu, route, det):
    """The loss gradient and the loss sum are the exact expected values first, then every gradient bit."""
    sat = xc.saturated()
    a = Abi(_model(gpu, "sat"), gpu)
    a.eng.set_deterministic(det)
    out = a.forward(sat.case)
    y = torch.from_numpy(sat.y.copy()).to(gpu)
    dl = torch.full((xc.SAT_B,), 7.0, device=gpu)
    loss = torch.zeros(1, device=gpu)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    if route == "bce_grad":
        a.lib.check(a.L.dfwfm_bce_grad(p(out), p(y), xc.SAT_B, float(xc.SAT_B), p(dl), p(loss), a.stream()), "bce")
        torch.cuda.synchronize()
        _assert_loss(route, dl.cpu().numpy(), float(loss.item()), sat)
        a.backward("whole", dl)
    else:
        first = a.lib.BWD_TILES if route == "bce-tiles-spread" else a.lib.BWD_TABLES | a.lib.BWD_MLP_WEIGHTS
        a.lib.check(a.L.dfwfm_backward_phases_bce(a.eng.handle, p(out), p(y), float(xc.SAT_B), p(dl), p(loss),
                                                  ctypes.byref(a.grads), first, a.stream()), "bwd bce")
        if route == "bce-tiles-spread":  # the tiles' losses are partials that SPREAD's REDUCE sums
            a.fork_spread(dl)
        torch.cuda.synchronize()
        _assert_loss(route, dl.cpu().numpy(), float(loss.item()), sat)
    _assert_bits(route, out.cpu().numpy(), a.result(), sat.case)


@pytest.mark.parametrize("mode", ["sorted", "atomic", "lazy_tables", "step_many"])
def test_saturated_fused_sgd_step(gpu, mode):
    """FusedTrainStep with plain SGD on a device-resident schedule: the eager first call and the capture call run at
    rate 0 and leave every parameter bit-identical; one replayed step at 2^-6 gives p - 2^-6 g of the float64
    reference bit for bit (lazy plain SGD: documented as the dense step's bits), with exact logits, dlogit and loss."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    sat = xc.saturated()
    case = sat.case
    m = build(case.cfg, _writable(case.params), gpu, is_deep_dropout=False)
    t = FusedTrainStep(m, xc.SAT_B, optimizer="sgd", momentum=0.0, weight_decay=0.0, lr_schedule=[(1, 0.0)],
                       deterministic=mode != "atomic", lazy_tables=mode == "lazy_tables",
                       resident_inputs=mode == "step_many")
    xi, xv, _ = _dev(gpu, case)
    y = torch.from_numpy(sat.y.copy()).to(gpu)
    step = (lambda: t.step_many([(xi, xv, y)])) if mode == "step_many" else (lambda: t.step(xi, xv, y))
    t.set_lr(0.0)
    t.step(xi, xv, y)  # eager
    step()             # captured, then replayed
    torch.cuda.synchronize()
    if mode == "step_many":  # the one-batch K-step graph was captured and replayed, not step()'s fallback
        assert len(t._many_sets) == 1 and t.graphs is None
    else:
        assert t.graphs is not None
    for k, q in m.named_parameters():
        assert np.array_equal(q.detach().cpu().numpy(), case.params[k]), (mode, k, "moved at rate 0")
    t.set_lr(xc.SGD_LR)
    t.loss_sum.zero_()  # (the trainer's loss sum runs over its steps)
    step()             # replayed
    torch.cuda.synchronize()
    assert len(t._many_sets) == (1 if mode == "step_many" else 0) and len(t._graph_sets) == (mode != "step_many")
    _assert_loss(mode, t.dlogit.cpu().numpy(), float(t.loss_sum.item()), sat)
    assert np.array_equal(t.out.cpu().numpy(), xc.ref32(case)[0]), (mode, "logits")
    want = xc.sgd_ref(sat)
    for k, q in m.named_parameters():
        got = q.detach().cpu().numpy()
        assert np.array_equal(got, want[k]), (mode, k, int(np.sum(got != want[k])), "elements differ")
    t.close()


@pytest.mark.parametrize("mode", ["sorted", "atomic", "lazy_tables", "step_many"])
def test_saturated_fused_sgd_step_with_dropout(gpu, mode):
    """The same with the model's default, deep-tower dropout 0.5, on, the rates on a device-resident schedule (0, 0,
    2^-6): step k draws its masks from step_seed(t.seed, k - 1), the trainer's device counter, in the forward and
    again in the per-tile backward.  The eager step's logits are the reference's under counter 0's masks and the
    captured step's under counter 1's (nothing moves at rate 0); after the third step every parameter is p - 2^-6 g
    of the float64 reference under counter 2's masks bit for bit, with exact logits, dlogit and loss.  step_many
    runs steps 2 and 3 as ONE graph over two resident batches.  The first time the dense non-Adam step runs with
    dropout."""
    import dp_cases as dc
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    sat0 = xc.saturated()
    case = sat0.case
    m = build(case.cfg, _writable(case.params), gpu, is_deep_dropout=True)
    t = FusedTrainStep(m, xc.SAT_B, optimizer="sgd", momentum=0.0, weight_decay=0.0,
                       lr_schedule=[(1, 0.0), (2, 0.0), (3, xc.SGD_LR), (4, 0.0)], deterministic=mode != "atomic",
                       lazy_tables=mode == "lazy_tables", resident_inputs=mode == "step_many")
    assert t.drop_train == 0.5
    sats = [dc.with_masks(sat0, dc.rank_masks(case.cfg, t.seed, k, xc.SAT_B)) for k in range(3)]
    assert max(xc.saturated_certificate(sats[2]).values()) < xc.LIMIT  # this seed's masks keep the witness's bound
    z = [xc.ref32(s.case)[0] for s in sats]
    assert not np.array_equal(z[0], z[1]) and not np.array_equal(z[1], z[2])
    xi, xv, _ = _dev(gpu, case)
    y = torch.from_numpy(sat0.y.copy()).to(gpu)
    t.step(xi, xv, y)  # eager, counter 0
    assert np.array_equal(t.out.cpu().numpy(), z[0]), (mode, "logits of the eager step")
    if mode == "step_many":  # counters 1 and 2 in one graph, on two resident buffer sets
        t.step_many([(xi, xv, y), (xi.clone(), xv.clone(), y.clone())])
        torch.cuda.synchronize()
        assert len(t._many_sets) == 1 and t.graphs is None
    else:
        t.step(xi, xv, y)  # captured, then replayed: counter 1
        assert np.array_equal(t.out.cpu().numpy(), z[1]), (mode, "logits of the captured step")
        for k, q in m.named_parameters():
            assert np.array_equal(q.detach().cpu().numpy(), case.params[k]), (mode, k, "moved at rate 0")
        t.loss_sum.zero_()  # (the trainer's loss sum runs over its steps)
        t.step(xi, xv, y)  # replayed: counter 2
        torch.cuda.synchronize()
        assert t.graphs is not None and len(t._graph_sets) == 1
        _assert_loss(mode, t.dlogit.cpu().numpy(), float(t.loss_sum.item()), sats[2])
    assert int(t.state[0].item()) == 3
    assert np.array_equal(t.out.cpu().numpy(), z[2]), (mode, "logits")
    assert np.array_equal(t.dlogit.cpu().numpy(), sat0.case.dlogit), (mode, "dlogit")
    want = xc.sgd_ref(sats[2])
    assert xc.differs(want, xc.sgd_ref(sat0))  # (dropout moved the update)
    for k, q in m.named_parameters():
        got = q.detach().cpu().numpy()
        assert np.array_equal(got, want[k]), (mode, k, int(np.sum(got != want[k])), "elements differ")
    t.close()
