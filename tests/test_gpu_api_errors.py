"""GPU: what the host side of the inference entry points (csrc/dfwfm_capi.hip) answers to a bad call -- the return
code and the full text of dfwfm_last_error(), and the order of the checks (which error wins, where nb = 0 or batch = 0
return OK).  The C functions are called raw through ctypes on two tiny models.  Every case ends in a host check:
nothing here launches a kernel beyond the models' setup (set_tables, set_dense, the packs, build_sparse_mlp).

The messages are the library's own, copied literally: a change of the host plumbing must not move one."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, STATE = 0, -1, -2, -4
B = 3
F, NUM, D, N = 3, 1, 10, 16
NC0 = -(-F * D // 16)

NO_TOWER = {
    "dfwfm_forward_gather": "forward_gather: the model has no deep tower",
    "dfwfm_serve_forward": "serve forward: the model has no deep tower (dfwfm_forward is one short launch)",
    "dfwfm_serve_workspace_bytes": "serve forward: the model has no deep tower",
    "dfwfm_bf16_forward": "bf16 forward: the model has no deep tower",
    "dfwfm_bf16_workspace_bytes": "bf16 forward: the model has no deep tower",
    "dfwfm_bf16_fused_forward": "bf16 fused forward: the model has no deep tower",
    "dfwfm_bf16_fused_forward_batches": "bf16 fused forward: the model has no deep tower",
    "dfwfm_int8_forward": "int8 forward: the model has no deep tower",
    "dfwfm_int8_forward_batches": "int8 forward: the model has no deep tower",
}
STALE = {
    "dfwfm_bf16_forward": "bf16 forward: the bf16 weight copy is absent or stale (dfwfm_model_pack_bf16)",
    "dfwfm_bf16_fused_forward": "bf16 fused forward: the bf16 weight copy is absent or stale (dfwfm_model_pack_bf16)",
    "dfwfm_bf16_fused_forward_batches":
        "bf16 fused forward: the bf16 weight copy is absent or stale (dfwfm_model_pack_bf16)",
    "dfwfm_int8_forward": "int8 forward: the int8 pack is absent or stale (dfwfm_model_pack_int8)",
    "dfwfm_int8_forward_batches": "int8 forward: the int8 pack is absent or stale (dfwfm_model_pack_int8)",
}
SHAPE = {
    "dfwfm_bf16_fused_forward_batches":
        "bf16 fused forward: shape not supported (embedding_size 10, field_size <= 48, deep_nodes <= 512, no "
        "FwFM pair list); use dfwfm_bf16_forward",
    "dfwfm_int8_forward_batches":
        "int8 forward: shape not supported (embedding_size 10, field_size <= 48, deep_nodes <= 512, no FwFM "
        "pair list)",
}
LONE = ("dfwfm_forward", "dfwfm_bf16_fused_forward", "dfwfm_int8_forward")       # (m, inputs, out, stream)
WITH_WS = ("dfwfm_forward_ws", "dfwfm_serve_forward", "dfwfm_bf16_forward")      # ... + workspace, ws_bytes
SETS = ("dfwfm_forward_batches", "dfwfm_bf16_fused_forward_batches", "dfwfm_int8_forward_batches")
WS_BYTES = {"dfwfm_forward_ws": "dfwfm_forward_workspace_bytes", "dfwfm_serve_forward": "dfwfm_serve_workspace_bytes",
            "dfwfm_bf16_forward": "dfwfm_bf16_workspace_bytes"}


def _cfg(deep, emb=D):
    return dict(field_size=F, numerical=NUM, embedding_size=emb, use_fwfm=1, use_fm=0, use_logit=0, use_deep=deep,
                use_lw=1, use_fwlw=0, h_depth=1 if deep else 0, deep_nodes=N if deep else 0)


class Model:
    """A ForwardEngine with its tables and dense parameters set from tensors kept here, and one batch of inputs."""

    def __init__(self, deep, device):
        from xsdeepfwfm_deprecated_amd.engine import ForwardEngine
        g = torch.Generator().manual_seed(5)

        def rnd(*shape):
            return (torch.rand(*shape, generator=g) - 0.5).to(device)

        self.device = device
        self.eng = ForwardEngine(_cfg(deep), device)
        self.h = self.eng.handle
        rows = [1] * NUM + [5] * (F - NUM)
        self.fields = [dict(emb2=rnd(n, D), emb2_r=None, emb1=rnd(n, 1), emb1_r=None, n=n, c=0, op=0) for n in rows]
        w1 = rnd(N, F * D)
        w1[torch.rand(N, F * D, generator=g).to(device) < 0.75] = 0  # a pruned layer, for build_sparse_mlp
        self.dense = (rnd(F, F), None, rnd(1, F), rnd(1), [w1] if deep else [], [rnd(N)] if deep else [],
                      rnd(1, N) if deep else None)
        self.eng.sync_tables(self.fields)
        self.eng.sync_dense(*self.dense)
        self.xi = torch.randint(0, 5, (B, F - NUM), generator=g).to(device)
        self.xv = torch.rand(B, NUM, generator=g).to(device)
        self.out = torch.empty(B, dtype=torch.float32, device=device)
        self.ws = torch.empty(1 << 16, dtype=torch.uint8, device=device)
        self.st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def inputs(self, batch=B):
        return (ctypes.c_void_p(self.xi.data_ptr()), self.xi.stride(0), ctypes.c_void_p(self.xv.data_ptr()),
                self.xv.stride(0), batch)

    def lone(self, name, batch=B, h="self", out="self"):
        """(rc, message) of a lone-batch forward; h / out: the handle and the output pointer, when not the model's."""
        h = self.h if h == "self" else h
        out = ctypes.c_void_p(self.out.data_ptr()) if out == "self" else out
        return _answer(getattr(_L(), name)(h, *self.inputs(batch), out, self.st))

    def with_ws(self, name, batch=B, ws="self", ws_bytes=None, h="self"):
        h = self.h if h == "self" else h
        ws = ctypes.c_void_p(self.ws.data_ptr()) if ws == "self" else ws
        ws_bytes = self.need(name, batch) if ws_bytes is None else ws_bytes
        return _answer(getattr(_L(), name)(h, *self.inputs(batch), ctypes.c_void_p(self.out.data_ptr()), ws, ws_bytes,
                                           self.st))

    def need(self, name, batch=B):
        n = ctypes.c_size_t(0)
        assert getattr(_L(), WS_BYTES[name])(self.h, batch, ctypes.byref(n)) == OK
        return n.value

    def batches(self, name, nb=2, batch=B, arrays=True, h="self"):
        h = self.h if h == "self" else h
        k = max(nb, 1)
        P = ctypes.c_void_p * k
        pxi, pxv, pout = (P(*[t.data_ptr()] * k) if arrays else None for t in (self.xi, self.xv, self.out))
        return _answer(getattr(_L(), name)(h, nb, pxi, self.xi.stride(0), pxv, self.xv.stride(0), batch, pout,
                                           self.st))

    def gather(self, batch=B, stride=NC0 * 16, h="self"):
        h = self.h if h == "self" else h
        return _answer(_L().dfwfm_forward_gather(h, *self.inputs(batch), ctypes.c_void_p(self.ws.data_ptr()), stride,
                                                 ctypes.c_void_p(self.out.data_ptr()), self.st))


def _L():
    from xsdeepfwfm_deprecated_amd import _lib
    return _lib.lib()


def _answer(rc):
    return rc, _L().dfwfm_last_error().decode()


@pytest.fixture(scope="module")
def deep(gpu):
    return Model(1, gpu)


@pytest.fixture(scope="module")
def packed(gpu):
    """The deep model with the bf16 copy, the int8 pack and the sparse deep tower in place."""
    m = Model(1, gpu)
    assert m.eng.sync_bf16(True) and m.eng.sync_int8(True)
    assert m.eng.sync_sparse(1.0)
    torch.cuda.synchronize()
    return m


@pytest.fixture(scope="module")
def shallow(gpu):
    return Model(0, gpu)


def test_null_model(deep):
    for name in LONE:
        assert deep.lone(name, h=None) == (INVALID, "null model")
    for name in WITH_WS:
        assert deep.with_ws(name, h=None, ws_bytes=0) == (INVALID, "null model")
    for name in SETS:
        assert deep.batches(name, h=None) == (INVALID, "null model")
    assert deep.gather(h=None) == (INVALID, "null model")
    L = _L()
    en, over, n = ctypes.c_int32(7), ctypes.c_int64(0), ctypes.c_size_t(0)
    assert _answer(L.dfwfm_model_pack_tables(None, 1, ctypes.byref(en), deep.st)) == (INVALID, "null argument")
    assert _answer(L.dfwfm_model_pack_tables_half(None, 1, ctypes.byref(en), ctypes.byref(over), deep.st)) == \
        (INVALID, "null argument")
    assert _answer(L.dfwfm_model_pack_tables(deep.h, 1, None, deep.st)) == (INVALID, "null argument")
    assert _answer(L.dfwfm_model_pack_bf16(None, 1, deep.st)) == (INVALID, "null model")
    assert _answer(L.dfwfm_model_pack_int8(None, deep.st)) == (INVALID, "null model")
    for name in ("dfwfm_forward_workspace_bytes", "dfwfm_serve_workspace_bytes", "dfwfm_bf16_workspace_bytes"):
        assert _answer(getattr(L, name)(None, B, ctypes.byref(n))) == (INVALID, "null argument")
        assert _answer(getattr(L, name)(deep.h, B, None)) == (INVALID, "null argument")
    assert _answer(L.dfwfm_serve_workspace_bytes(deep.h, -1, ctypes.byref(n))) == (INVALID, "negative batch")
    assert _answer(L.dfwfm_bf16_workspace_bytes(deep.h, -1, ctypes.byref(n))) == (INVALID, "negative batch")
    assert _answer(L.dfwfm_forward_workspace_bytes(deep.h, -1, ctypes.byref(n))) == (INVALID, "null argument")


def test_batch_sets_argument_checks(packed):
    for name in SETS:
        assert packed.batches(name, nb=-1) == (INVALID, "negative batch count")
        assert packed.batches(name, nb=2, arrays=False) == (INVALID, "null pointer array")
        assert packed.batches(name, nb=2, batch=-1) == (INVALID, "negative batch")
        # no batch and no row: OK, also without pointer arrays when there is no batch
        assert packed.batches(name, nb=0, arrays=False)[0] == OK
        assert packed.batches(name, nb=0, batch=-1)[0] == OK
        assert packed.batches(name, nb=2, batch=0)[0] == OK
    # a null pointer inside the array is the lone forward's message
    P = ctypes.c_void_p * 2
    good = P(packed.out.data_ptr(), packed.out.data_ptr())
    for name in SETS:
        rc = getattr(_L(), name)(packed.h, 2, P(packed.xi.data_ptr(), packed.xi.data_ptr()), packed.xi.stride(0),
                                 P(packed.xv.data_ptr(), packed.xv.data_ptr()), packed.xv.stride(0), B,
                                 P(packed.out.data_ptr(), None), packed.st)
        assert _answer(rc) == (INVALID, "null input/output pointer"), name
        rc = getattr(_L(), name)(packed.h, 2, P(packed.xi.data_ptr(), packed.xi.data_ptr()), 1,
                                 P(packed.xv.data_ptr(), packed.xv.data_ptr()), packed.xv.stride(0), B, good,
                                 packed.st)
        assert _answer(rc) == (INVALID, "xi_stride < F - numerical"), name


def test_lone_forwards_argument_checks(packed):
    for name in LONE:
        assert packed.lone(name, batch=-1) == (INVALID, "negative batch")
        assert packed.lone(name, out=None) == (INVALID, "null input/output pointer")
        assert packed.lone(name, batch=0)[0] == OK
        assert packed.lone(name, batch=0, out=None)[0] == OK
    for name in WITH_WS:
        assert packed.with_ws(name, batch=-1, ws_bytes=0) == (INVALID, "negative batch")
        assert packed.with_ws(name, batch=0, ws_bytes=0)[0] == OK
        assert packed.with_ws(name, batch=0, ws=None, ws_bytes=0)[0] == OK
    assert packed.gather(batch=-1) == (INVALID, "negative batch")
    assert packed.gather(batch=0)[0] == OK


def test_forward_before_the_pack(deep):
    """The copy the forward reads is absent: a state error, which also wins over batch = 0; nb = 0 and the argument
    checks come first."""
    for name in ("dfwfm_bf16_fused_forward", "dfwfm_int8_forward"):
        assert deep.lone(name) == (STATE, STALE[name])
        assert deep.lone(name, batch=0) == (STATE, STALE[name])
        assert deep.lone(name, batch=-1) == (INVALID, "negative batch")
        assert deep.lone(name, out=None) == (INVALID, "null input/output pointer")
    for name in ("dfwfm_bf16_fused_forward_batches", "dfwfm_int8_forward_batches"):
        assert deep.batches(name) == (STATE, STALE[name])
        assert deep.batches(name, batch=0) == (STATE, STALE[name])
        assert deep.batches(name, nb=0)[0] == OK
        assert deep.batches(name, arrays=False) == (INVALID, "null pointer array")
    name = "dfwfm_bf16_forward"
    assert deep.with_ws(name) == (STATE, STALE[name])
    assert deep.with_ws(name, batch=0, ws_bytes=0) == (STATE, STALE[name])
    assert deep.with_ws(name, ws=None, ws_bytes=0) == (STATE, STALE[name])
    assert deep.with_ws(name, batch=-1, ws_bytes=0) == (INVALID, "negative batch")


def test_no_deep_tower(shallow):
    """The FwFM-only model: refused before any other check but the null model and the batch count."""
    n = ctypes.c_size_t(0)
    for name in ("dfwfm_bf16_fused_forward", "dfwfm_int8_forward"):
        assert shallow.lone(name) == (UNSUPPORTED, NO_TOWER[name])
        assert shallow.lone(name, batch=-1) == (UNSUPPORTED, NO_TOWER[name])
    for name in ("dfwfm_bf16_fused_forward_batches", "dfwfm_int8_forward_batches"):
        assert shallow.batches(name) == (UNSUPPORTED, NO_TOWER[name])
        assert shallow.batches(name, nb=0) == (UNSUPPORTED, NO_TOWER[name])
        assert shallow.batches(name, nb=-1) == (INVALID, "negative batch count")
    for name in ("dfwfm_serve_forward", "dfwfm_bf16_forward"):
        assert shallow.with_ws(name, ws_bytes=1 << 16) == (UNSUPPORTED, NO_TOWER[name])
        assert shallow.with_ws(name, batch=0, ws=None, ws_bytes=0) == (UNSUPPORTED, NO_TOWER[name])
        assert _answer(getattr(_L(), WS_BYTES[name])(shallow.h, B, ctypes.byref(n))) == \
            (UNSUPPORTED, NO_TOWER[WS_BYTES[name]])
    assert shallow.gather() == (UNSUPPORTED, NO_TOWER["dfwfm_forward_gather"])
    assert shallow.gather(batch=-1) == (UNSUPPORTED, NO_TOWER["dfwfm_forward_gather"])
    assert _answer(_L().dfwfm_model_pack_bf16(shallow.h, 1, shallow.st)) == \
        (UNSUPPORTED, "bf16 pack: the model has no deep tower")
    assert _answer(_L().dfwfm_model_pack_bf16(shallow.h, 0, shallow.st))[0] == OK
    assert _answer(_L().dfwfm_model_pack_int8(shallow.h, shallow.st)) == \
        (UNSUPPORTED, "int8 pack: the model has no deep tower")
    # without a sparse tower dfwfm_forward_ws is dfwfm_forward and needs no workspace
    assert _answer(_L().dfwfm_forward_workspace_bytes(shallow.h, B, ctypes.byref(n)))[0] == OK and n.value == 0
    assert shallow.with_ws("dfwfm_forward_ws", batch=-1, ws=None, ws_bytes=0) == (INVALID, "negative batch")


def test_unsupported_shape(gpu):
    """embedding_size 8: the one-launch forwards refuse the shape before they look at the batches or the state."""
    from xsdeepfwfm_deprecated_amd.engine import ForwardEngine
    eng = ForwardEngine(_cfg(1, emb=8), gpu)
    P = ctypes.c_void_p * 1
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    for name, text in SHAPE.items():
        assert _answer(getattr(_L(), name)(eng.handle, 1, P(), 0, P(), 0, B, P(), st)) == (UNSUPPORTED, text)
        assert _answer(getattr(_L(), name)(eng.handle, 0, None, 0, None, 0, B, None, st)) == (UNSUPPORTED, text)
    v = ctypes.c_int(1)
    assert _L().dfwfm_bf16_fused_supported(eng.handle, ctypes.byref(v)) == OK and v.value == 0
    v = ctypes.c_int(1)
    assert _L().dfwfm_int8_supported(eng.handle, ctypes.byref(v)) == OK and v.value == 0
    assert _answer(_L().dfwfm_model_pack_int8(eng.handle, st)) == \
        (UNSUPPORTED, "int8 pack: shape not supported (embedding_size 10, field_size <= 48, deep_nodes <= 512)")
    eng.close()


def test_workspace_checks(packed):
    for name in WITH_WS:
        need = packed.need(name)
        assert need > 0, name
        assert packed.with_ws(name, ws_bytes=need - 1) == \
            (INVALID, f"workspace of {need - 1} bytes < {need} ({WS_BYTES[name]})"), name
        assert packed.with_ws(name, ws=ctypes.c_void_p(packed.ws.data_ptr() + 4)) == \
            (INVALID, "workspace not 16-byte aligned"), name
        # the size is checked before the alignment
        assert packed.with_ws(name, ws=ctypes.c_void_p(packed.ws.data_ptr() + 4), ws_bytes=0) == \
            (INVALID, f"workspace of 0 bytes < {need} ({WS_BYTES[name]})"), name
    assert packed.need("dfwfm_forward_ws") == 4 * B * (NC0 * 16 + 1)
    for name in ("dfwfm_serve_forward", "dfwfm_bf16_forward"):
        assert packed.with_ws(name, ws=None) == (INVALID, "null workspace"), name
        assert packed.with_ws(name, ws=None, batch=-1, ws_bytes=0) == (INVALID, "negative batch"), name


def test_forward_gather_checks(packed):
    assert packed.gather(stride=NC0 * 16 - 1) == (INVALID, f"deep_emb stride {NC0 * 16 - 1}, need {NC0 * 16}")
    L = _L()
    rc = L.dfwfm_forward_gather(packed.h, *packed.inputs(), None, NC0 * 16, ctypes.c_void_p(packed.out.data_ptr()),
                                packed.st)
    assert _answer(rc) == (INVALID, f"deep_emb stride {NC0 * 16}, need {NC0 * 16}")
    rc = L.dfwfm_forward_gather(packed.h, *packed.inputs(), ctypes.c_void_p(packed.ws.data_ptr() + 4), NC0 * 16,
                                ctypes.c_void_p(packed.out.data_ptr()), packed.st)
    assert _answer(rc) == (INVALID, "deep_emb not 16-byte aligned")
    rc = L.dfwfm_forward_gather(packed.h, *packed.inputs(), ctypes.c_void_p(packed.ws.data_ptr()), NC0 * 16, None,
                                packed.st)
    assert _answer(rc) == (INVALID, "null input/output pointer")


def test_before_set_tables(gpu):
    from xsdeepfwfm_deprecated_amd.engine import ForwardEngine
    eng = ForwardEngine(_cfg(1), gpu)
    L = _L()
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    en, over = ctypes.c_int32(7), ctypes.c_int64(7)
    assert _answer(L.dfwfm_model_pack_tables(eng.handle, 1, ctypes.byref(en), st)) == \
        (STATE, "set_tables must precede pack_tables")
    assert en.value == 0
    en = ctypes.c_int32(7)
    assert _answer(L.dfwfm_model_pack_tables_half(eng.handle, 1, ctypes.byref(en), ctypes.byref(over), st)) == \
        (STATE, "set_tables must precede pack_tables_half")
    assert en.value == 0 and over.value == 0
    assert L.dfwfm_model_pack_tables(eng.handle, 0, ctypes.byref(en), st) == OK  # turning it off needs no table
    assert L.dfwfm_model_pack_tables_half(eng.handle, 0, ctypes.byref(en), None, st) == OK
    assert _answer(L.dfwfm_model_pack_bf16(eng.handle, 1, st)) == (STATE, "set_dense must precede pack_bf16")
    assert _answer(L.dfwfm_model_pack_int8(eng.handle, st)) == (STATE, "set_dense must precede pack_int8")
    x = ctypes.c_void_p(16)  # never read: the state check comes before any use of the pointers
    msg = "set_tables and set_dense must precede forward"
    assert _answer(L.dfwfm_forward(eng.handle, x, 2, x, 1, B, x, st)) == (STATE, msg)
    assert _answer(L.dfwfm_forward(eng.handle, x, 2, x, 1, 0, x, st)) == (STATE, msg)
    assert _answer(L.dfwfm_serve_forward(eng.handle, x, 2, x, 1, B, x, x, 1 << 20, st)) == (STATE, msg)
    assert _answer(L.dfwfm_bf16_forward(eng.handle, x, 2, x, 1, B, x, x, 1 << 20, st)) == (STATE, msg)
    assert _answer(L.dfwfm_bf16_fused_forward(eng.handle, x, 2, x, 1, B, x, st)) == (STATE, msg)
    assert _answer(L.dfwfm_int8_forward(eng.handle, x, 2, x, 1, B, x, st)) == (STATE, msg)
    assert _answer(L.dfwfm_forward_gather(eng.handle, x, 2, x, 1, B, x, NC0 * 16, x, st)) == (STATE, msg)
    eng.close()


def test_adam_tensor_lists(gpu):
    from xsdeepfwfm_deprecated_amd import _lib
    L = _L()
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    t = torch.zeros(8, dtype=torch.float32, device=gpu)
    state = torch.zeros(_lib.ADAM_STATE_BYTES, dtype=torch.uint8, device=gpu)
    p = t.data_ptr()
    arr = (_lib.dfwfm_adam_tensor * 2)(_lib.dfwfm_adam_tensor(p, None, None, None, 8),  # no grad: skipped
                                       _lib.dfwfm_adam_tensor(p, p, None, p, 8))
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert _answer(L.dfwfm_adam_step(arr, 2, *hyper, 1, st)) == (INVALID, "adam tensor 1: null state pointer")
    assert _answer(L.dfwfm_adam_step_dev(arr, 2, *hyper, ctypes.c_void_p(state.data_ptr()), st)) == \
        (INVALID, "adam tensor 1: null state pointer")
    assert _answer(L.dfwfm_adam_step(None, 2, *hyper, 1, st)) == (INVALID, "null tensor list")
    assert _answer(L.dfwfm_adam_step(arr, -1, *hyper, 1, st)) == (INVALID, "negative tensor count")
    assert _answer(L.dfwfm_adam_step(arr, 1, *hyper, 0, st)) == (INVALID, "step must be >= 1")
    assert _answer(L.dfwfm_adam_step_dev(None, 2, *hyper, ctypes.c_void_p(state.data_ptr()), st)) == \
        (INVALID, "null argument")
    assert _answer(L.dfwfm_adam_step_dev(arr, 2, *hyper, None, st)) == (INVALID, "null argument")
    assert _answer(L.dfwfm_adam_step_dev(arr, -1, *hyper, ctypes.c_void_p(state.data_ptr()), st)) == \
        (INVALID, "negative tensor count")
    assert L.dfwfm_adam_step(arr, 0, *hyper, 1, st) == OK  # no tensor: no launch


@pytest.mark.parametrize("method", ["forward", "forward_small", "forward_bf16"])
def test_output_smaller_than_the_batch(packed, method):
    """An `out` of B - 1 elements is refused before the C call, as forward_bf16_fused and forward_int8 refuse it.
    This is the one test of this file that fails on the commit before the host plumbing was shared: these three
    handed the short tensor to the kernel."""
    eng = packed.eng
    assert eng.small_rows == 0 and not eng.bf16 and not eng.int8  # forward() itself, not one of its routes
    short = torch.empty(B - 1, dtype=torch.float32, device=packed.device)
    with pytest.raises(ValueError, match="smaller"):
        getattr(eng, method)(packed.xi, packed.xv, short)
    for other in ("forward_bf16_fused", "forward_int8"):
        with pytest.raises(ValueError, match="smaller"):
            getattr(eng, other)(packed.xi, packed.xv, short)
