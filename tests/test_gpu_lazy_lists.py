"""GPU: the list-driven row-lazy steps (include/dfwfm_lazy_lists.h), one process, no process group.

The call alone on a hand-built flat buffer: spans (1, 10), (7, 10), (7, 1), (5000, 10), (5000, 1) at 4-float-padded
offsets, W = 1, 2 and 8 lists per width, disjoint / identical / randomly overlapping lists, counts 0, 1, exactly cap
and cap + 5 over cap valid entries, the first and last row of the first and last span.  Expected: array_equal to the
dense kernel (dfwfm_adam_step / dfwfm_optim_step at the explicit step number) run on the union rows gathered into
compact tensors, for Adam, plain SGD, momentum-SGD, Adagrad and RMSprop (and dfwfm_optim_elem_ref on them); untouched
rows and the pads bit-unchanged, touched gradient rows zero, the counter advanced by exactly one, also with all-empty
lists.  Then: the global step over three calls, the scheduled entries, graph capture, run-to-run identity, and more
spans and lists than one launch takes."""
import ctypes

import numpy as np
import pytest
import torch

import lazy_lists_ref as ref
import optim_ref

pytestmark = pytest.mark.gpu

LR, WD, BETAS, EPS = 1e-3, 3e-7, (0.9, 0.999), 1e-8
KINDS = [("adam", 0.0), ("sgd", 0.0), ("sgd", 0.9), ("adag", 0.0), ("rmsp", 0.0)]
IDS = ["adam", "sgd", "sgd-momentum", "adag", "rmsp"]
SHAPES = [(1, 10), (7, 10), (7, 1), (5000, 10), (5000, 1)]
SPANS_PER_LAUNCH, LISTS_PER_LAUNCH = 64, 32  # include/dfwfm_lazy_lists.h


def _stream(gpu):
    return ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


def _layout(shapes):
    """Spans (offset, rows, width) at 4-float-padded offsets, and the flat buffers' length."""
    spans, off = [], 0
    for rows, width in shapes:
        spans.append((off, rows, width))
        off += (rows * width + 3) & ~3
    return spans, off


def _buffers(kind, spans, total, seed, gpu):
    """Random tables, a flat gradient (magnitudes 1e-8 .. 1, the pads included) and flat moments / state as after
    earlier steps (m signed, v >= 0; a sum / square_avg >= 0; none for plain SGD), zero stamps."""
    opt, mom = kind
    r = np.random.default_rng(seed)
    b = {"p": [torch.from_numpy(r.standard_normal((rows, w)).astype(np.float32)).to(gpu) for _, rows, w in spans],
         "stamp": [torch.zeros(rows, dtype=torch.int32, device=gpu) for _, rows, _ in spans]}
    g = (r.standard_normal(total) * 10.0 ** r.uniform(-8, 0, total)).astype(np.float32)
    m = (0.1 * r.standard_normal(total)).astype(np.float32)
    v = (0.01 * r.random(total)).astype(np.float32)
    b["g"] = torch.from_numpy(g).to(gpu)
    b["m"] = b["v"] = None
    if opt == "adam":
        b["m"], b["v"] = torch.from_numpy(m).to(gpu), torch.from_numpy(v).to(gpu)
    elif optim_ref.has_state(opt, mom):
        b["m"] = torch.from_numpy(m if opt == "sgd" else np.abs(m)).to(gpu)
    return b


def _clone(b):
    return {k: ([t.clone() for t in v] if isinstance(v, list) else (None if v is None else v.clone()))
            for k, v in b.items()}


def _new_state(gpu, step_before=0):
    from xsdeepfwfm_deprecated_amd import _lib
    st = torch.zeros(_lib.ADAM_STATE_BYTES // 8, dtype=torch.int64, device=gpu)
    st[0] = step_before
    return st


def _dev_lists(lists, gpu):
    """Host lists (dest, count, cap, width) on the device: dest [cap] int64, count [1] int32."""
    out = []
    for dest, count, cap, width in lists:
        assert len(dest) == cap
        out.append((torch.from_numpy(np.asarray(dest, np.int64).copy()).to(gpu),
                    torch.tensor([count], dtype=torch.int32, device=gpu), cap, width))
    return out


def _call(kind, b, spans, dl, state, gpu, wd=WD, lr=LR, sched=None):
    from xsdeepfwfm_deprecated_amd import _lib
    opt, mom = kind
    L, P = _lib.lib(), ctypes.c_void_p
    sa = (_lib.dfwfm_lazy_lists_span * max(len(spans), 1))()
    for i, (off, rows, w) in enumerate(spans):
        sa[i] = _lib.dfwfm_lazy_lists_span(b["p"][i].data_ptr(), b["stamp"][i].data_ptr(), off, rows, w, 0)
    la = (_lib.dfwfm_lazy_lists_list * max(len(dl), 1))()
    for i, (dest, count, cap, w) in enumerate(dl):
        la[i] = _lib.dfwfm_lazy_lists_list(dest.data_ptr(), count.data_ptr(), cap, w, 0)
    g, st = P(b["g"].data_ptr()), P(state.data_ptr())
    m = None if b["m"] is None else P(b["m"].data_ptr())
    if opt == "adam":
        v = P(b["v"].data_ptr())
        if sched is not None:
            _lib.check(L.dfwfm_lazy_adam_lists_step_dev_sched(sa, len(spans), la, len(dl), g, m, v, P(sched.data_ptr()),
                                                              BETAS[0], BETAS[1], EPS, wd, st, _stream(gpu)), "lists")
        else:
            _lib.check(L.dfwfm_lazy_adam_lists_step_dev(sa, len(spans), la, len(dl), g, m, v, lr, BETAS[0], BETAS[1],
                                                        EPS, wd, st, _stream(gpu)), "lists")
        return
    h = optim_ref.hyper(opt, lr, wd, mom)
    if sched is not None:
        _lib.check(L.dfwfm_lazy_optim_lists_step_dev_sched(sa, len(spans), la, len(dl), g, m, ctypes.byref(h),
                                                           P(sched.data_ptr()), st, _stream(gpu)), "lists")
    else:
        _lib.check(L.dfwfm_lazy_optim_lists_step_dev(sa, len(spans), la, len(dl), g, m, ctypes.byref(h), st,
                                                     _stream(gpu)), "lists")


def _dense_on_union(kind, b, spans, lists, step, gpu, wd=WD, lr=LR):
    """Expected buffers after the lists step `step`: per span the union rows (tests/lazy_lists_ref.py) gathered into
    compact tensors, the dense kernel (explicit step number) run on them, scattered back, their gradient zeroed.  b is
    updated in place; returns the union rows per span."""
    from xsdeepfwfm_deprecated_amd import _lib, engine
    opt, mom = kind
    union = ref.union_rows(spans, lists)
    for i, ((off, rows, w), touched) in enumerate(zip(spans, union)):
        if not len(touched):
            continue
        idx = torch.from_numpy(touched).to(gpu)
        view = lambda t: t[off:off + rows * w].view(rows, w)  # noqa: E731
        pc, gc = b["p"][i][idx].contiguous(), view(b["g"])[idx].contiguous()
        mc = None if b["m"] is None else view(b["m"])[idx].contiguous()
        if opt == "adam":
            vc = view(b["v"])[idx].contiguous()
            engine.adam_step([(pc, gc, mc, vc)], lr, BETAS[0], BETAS[1], EPS, wd, step, gpu)
            view(b["v"])[idx] = vc
        else:
            arr = (_lib.dfwfm_optim_tensor * 1)(_lib.dfwfm_optim_tensor(
                pc.data_ptr(), gc.data_ptr(), None if mc is None else mc.data_ptr(), pc.numel()))
            h = optim_ref.hyper(opt, lr, wd, mom)
            _lib.check(_lib.lib().dfwfm_optim_step(arr, 1, ctypes.byref(h), int(step), _stream(gpu)),
                       "dfwfm_optim_step")
        b["p"][i][idx] = pc
        if mc is not None:
            view(b["m"])[idx] = mc
        view(b["g"])[idx] = 0.0
    return union


def _same(got, want, what=""):
    for k in ("g", "m", "v"):
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), (what, k)
    for i, (a, c) in enumerate(zip(got["p"], want["p"])):
        assert np.array_equal(a.cpu().numpy(), c.cpu().numpy()), (what, "p", i)


def _check_call(kind, spans, total, lists, gpu, seed=3, step_before=0, wd=WD):
    """One call from random buffers against the dense kernel on the union rows, with everything around it."""
    b = _buffers(kind, spans, total, seed, gpu)
    want, before = _clone(b), _clone(b)
    state = _new_state(gpu, step_before)
    _call(kind, b, spans, _dev_lists(lists, gpu), state, gpu, wd=wd)
    torch.cuda.synchronize()
    assert int(state[0].item()) == step_before + 1 and int(state.view(torch.int32)[9].item()) == 0  # counter, ticket
    union = _dense_on_union(kind, want, spans, lists, step_before + 1, gpu, wd=wd)
    _same(b, want, kind)
    g0, g1 = before["g"].cpu().numpy(), b["g"].cpu().numpy()
    keep = np.ones(total, bool)
    for i, ((off, rows, w), touched) in enumerate(zip(spans, union)):
        rest = np.setdiff1d(np.arange(rows), touched)
        assert np.array_equal(b["p"][i].cpu().numpy()[rest], before["p"][i].cpu().numpy()[rest])  # every bit kept
        assert not g1[off:off + rows * w].reshape(rows, w)[touched].any()
        assert np.array_equal(np.flatnonzero(b["stamp"][i].cpu().numpy()), touched)  # claimed exactly the union
        keep[off:off + rows * w].reshape(rows, w)[touched] = False
    assert np.array_equal(g1[keep], g0[keep])  # untouched gradient rows and the pads
    for k in ("m", "v"):
        if b[k] is not None:
            assert np.array_equal(b[k].cpu().numpy()[keep], before[k].cpu().numpy()[keep]), k
    return b, before, union


def _pool(spans, width, n, seed):
    """Up to n distinct destinations of rows in the spans of `width`: always the first and the last row of every such
    span (so of the first and of the last span of all), the rest random."""
    r = np.random.default_rng(seed)
    mine = [(off, rows) for off, rows, w in spans if w == width]
    forced = sorted({d for off, rows in mine for d in (off, off + (rows - 1) * width)})
    every = np.concatenate([off + width * np.arange(rows, dtype=np.int64) for off, rows in mine])
    rest = np.setdiff1d(every, np.fromiter(forced, np.int64))
    take = r.permutation(rest)[:max(0, min(n, len(every)) - len(forced))]
    forced = np.fromiter(forced, np.int64)
    return r.permutation(np.concatenate([forced, take])), np.setdiff1d(rest, take), forced


def _pattern_lists(spans, pattern, W, seed):
    """W lists per width.  Behind each list's count sit `spare` destinations of rows no list names (they must stay
    untouched: the reader stops at the count)."""
    lists = []
    for width in (10, 1):
        pool, spare, forced = _pool(spans, width, 330, seed + width)
        r = np.random.default_rng(seed + 7 * width)
        for k in range(W):
            if pattern == "disjoint":
                d = pool[k::W]
            elif pattern == "same":
                d = pool
            else:
                d = pool[(r.random(len(pool)) < 0.5) | np.isin(pool, forced)]
            tail = spare[:3]
            lists.append((np.concatenate([d, tail]), len(d), len(d) + len(tail), width))
    return lists


# ------------------------------------------------------------------------------------------------ the call alone
@pytest.mark.parametrize("pattern", ["disjoint", "same", "random"])
@pytest.mark.parametrize("W", [1, 2, 8])
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_lists_call_equals_dense_kernel_on_union_rows(gpu, kind, W, pattern):
    """The five spans, W lists per width (2 W lists), at step 2 (no variant's first step): every tensor bit for bit
    against the dense kernel on the union rows; the first and last row of the first and last span are listed."""
    spans, total = _layout(SHAPES)
    lists = _pattern_lists(spans, pattern, W, 40 + W)
    _, _, union = _check_call(kind, spans, total, lists, gpu, step_before=1)
    assert union[0].tolist() == [0] and {0, 6} <= set(union[2].tolist())
    assert {0, 4999} <= set(union[3].tolist()) and {0, 4999} <= set(union[4].tolist())
    assert sum(len(u) for u in union) > 300
    if pattern == "same" and W > 1:  # every row named W times, updated once
        assert sum(len(u) for u in union) * W == sum(c for _, c, _, _ in lists)


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_counts_zero_one_cap_and_past_cap(gpu, kind):
    """Per width four lists: count 0 (its entries must not be read), 1, exactly cap, and cap + 5 over cap valid entries
    (the reader stops at cap); a negative count reads nothing.  Also against dfwfm_optim_elem_ref on the host."""
    spans, total = _layout(SHAPES)
    lists = []
    for width in (10, 1):
        pool = _pool(spans, width, 40, 5 + width)[0]
        lists += [(pool[0:6], 0, 6, width), (pool[6:12], 1, 6, width), (pool[12:20], 8, 8, width),
                  (pool[20:31], 16, 11, width), (pool[31:35], -2, 4, width)]
    b, before, union = _check_call(kind, spans, total, lists, gpu, step_before=1)
    assert sum(len(u) for u in union) == 2 * (1 + 8 + 11)
    opt, mom = kind
    if opt != "adam":
        host = lambda x: None if x is None else x.cpu().numpy()  # noqa: E731
        hp, hg, hs = ref.lazy_optim_lists_ref(opt, [host(p) for p in before["p"]], host(before["g"]),
                                              host(before["m"]), spans, lists, 2, lr=LR, weight_decay=WD,
                                              momentum=mom, elem="lib")
        for a, c in zip(b["p"], hp):
            assert optim_ref.same_bits(host(a), c)
        assert optim_ref.same_bits(host(b["g"]), hg) and (hs is None or optim_ref.same_bits(host(b["m"]), hs))


@pytest.mark.parametrize("kind", [KINDS[0], KINDS[3]], ids=["adam", "adag"])
def test_empty_lists_advance_the_counter_only(gpu, kind):
    """All counts zero, no list, no span: nothing changes and the counter advances by exactly one per call."""
    spans, total = _layout(SHAPES)
    b = _buffers(kind, spans, total, 8, gpu)
    want = _clone(b)
    state = _new_state(gpu)
    pool = _pool(spans, 10, 12, 1)[0]
    _call(kind, b, spans, _dev_lists([(pool, 0, len(pool), 10), (pool, 0, len(pool), 10)], gpu), state, gpu)
    _call(kind, b, spans, [], state, gpu)
    _call(kind, b, [], [], state, gpu)
    torch.cuda.synchronize()
    assert int(state[0].item()) == 3
    _same(b, want)
    assert not any(s.any().item() for s in b["stamp"])


@pytest.mark.parametrize("kind", [KINDS[1], KINDS[4]], ids=["sgd", "rmsp"])
def test_destinations_in_no_span_are_skipped(gpu, kind):
    """Destinations in a pad, between two rows, in a span of another width, below the first span's offset, past the
    last span and negative: not written, not an error; the valid ones beside them are updated."""
    spans, total = _layout(SHAPES)
    spans = [(off + 16, rows, w) for off, rows, w in spans]  # nothing at floats 0 .. 15
    total += 16
    o = [s[0] for s in spans]
    lists = [(np.array([o[1] + 20, o[0] + 10, o[1] + 5, o[2], 0, 8, total, 2 ** 40, -10, o[3] + 49990], np.int64),
              10, 10, 10),
             (np.array([o[2] + 3, o[2] + 7, o[1], o[4] + 5000, -1, o[4]], np.int64), 6, 6, 1)]
    _, _, union = _check_call(kind, spans, total, lists, gpu)
    assert [u.tolist() for u in union] == [[], [2], [3], [4999], [0]]


@pytest.mark.parametrize("kind", [KINDS[0], KINDS[2]], ids=["adam", "sgd-momentum"])
def test_three_calls_use_the_global_step(gpu, kind):
    """Row 3 of the (7, 10) span is listed at steps 1 and 3 only: it keeps its bits at step 2 and gets step 3's
    coefficients at step 3 (the dense kernel at the explicit steps on the union rows, from zero moments / state)."""
    spans, total = _layout(SHAPES)
    b = _buffers(kind, spans, total, 21, gpu)
    for k in ("m", "v"):
        if b[k] is not None:
            b[k].zero_()
    want = _clone(b)
    o = spans[1][0]
    calls = [[(np.array([o + 30, o + 50], np.int64), 2, 2, 10)],
             [(np.array([o + 10, o + 50], np.int64), 2, 2, 10)],
             [(np.array([o + 30], np.int64), 1, 1, 10), (np.array([o + 30, o], np.int64), 2, 2, 10)]]
    state = _new_state(gpu)
    row3 = []
    for s, lists in enumerate(calls, 1):
        g = _buffers(kind, spans, total, 30 + s, gpu)["g"]
        for x in (b, want):
            x["g"].copy_(g)
        _call(kind, b, spans, _dev_lists(lists, gpu), state, gpu)
        _dense_on_union(kind, want, spans, lists, s, gpu)
        _same(b, want, s)
        row3.append(b["p"][1][3].cpu().numpy().copy())
    assert int(state[0].item()) == 3
    assert np.array_equal(row3[0], row3[1]) and not np.array_equal(row3[1], row3[2])


@pytest.mark.parametrize("kind", [KINDS[0], KINDS[4]], ids=["adam", "rmsp"])
def test_scheduled_call_equals_the_unscheduled_call_at_the_schedules_rate(gpu, kind):
    """At steps 2 (inside a segment), 3 (a knot) and 7 (past the last knot) the scheduled entry gives the bits of the
    unscheduled entry with lr = dfwfm_lr_schedule_eval(step)."""
    from xsdeepfwfm_deprecated_amd import _lib
    spans, total = _layout(SHAPES)
    lists = _pattern_lists(spans, "random", 2, 77)
    knots = [(1, 1e-4), (3, 1e-3), (6, 2e-4)]
    sched = torch.zeros(_lib.LR_SCHEDULE_BYTES // 8, dtype=torch.int64, device=gpu)
    arr, n = _lib.lr_knots(knots)
    _lib.check(_lib.lib().dfwfm_lr_schedule_write(ctypes.c_void_p(sched.data_ptr()), arr, n, _stream(gpu)), "write")
    rates = set()
    for step in (2, 3, 7):
        lr = _lib.lr_schedule_eval(knots, step)
        rates.add(lr)
        a, c = _buffers(kind, spans, total, 60, gpu), _buffers(kind, spans, total, 60, gpu)
        sa, sc = _new_state(gpu, step - 1), _new_state(gpu, step - 1)
        _call(kind, a, spans, _dev_lists(lists, gpu), sa, gpu, lr=123.0, sched=sched)  # lr unused
        _call(kind, c, spans, _dev_lists(lists, gpu), sc, gpu, lr=lr)
        _same(a, c, step)
        assert int(sa[0].item()) == int(sc[0].item()) == step
    assert len(rates) == 3


@pytest.mark.parametrize("kind", [KINDS[0], KINDS[3]], ids=["adam", "adag"])
def test_captured_call_replayed_three_times_equals_three_eager_calls(gpu, kind):
    """One captured call, replayed with new destinations, counts and gradients written into the same buffers between
    replays: counts, destinations, gradients and the counter are read afresh."""
    spans, total = _layout(SHAPES)
    steps = [_pattern_lists(spans, p, 2, 90 + i) for i, p in enumerate(("random", "disjoint", "same"))]
    cap = {w: max(l[2] for ls in steps for l in ls if l[3] == w) for w in (10, 1)}
    dl = [(torch.zeros(cap[w], dtype=torch.int64, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu), cap[w], w)
          for _, _, _, w in steps[0]]
    grads = [_buffers(kind, spans, total, 100 + s, gpu)["g"] for s in range(3)]

    def load(lists):
        for (dest, count, _, _), (d, c, _, _) in zip(dl, lists):
            dest[:len(d)].copy_(torch.from_numpy(np.asarray(d, np.int64).copy()))
            count.fill_(c)

    a, c = _buffers(kind, spans, total, 61, gpu), _buffers(kind, spans, total, 61, gpu)
    sa, sc = _new_state(gpu), _new_state(gpu)
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    load(steps[0])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            _call(kind, a, spans, dl, sa, gpu)
    torch.cuda.current_stream(gpu).wait_stream(s)
    assert int(sa[0].item()) == 0  # captured, not run
    for lists, g in zip(steps, grads):
        load(lists)
        a["g"].copy_(g)
        graph.replay()
        c["g"].copy_(g)
        _call(kind, c, spans, _dev_lists(lists, gpu), sc, gpu)
    torch.cuda.synchronize()
    _same(a, c)
    assert int(sa[0].item()) == int(sc[0].item()) == 3


@pytest.mark.parametrize("kind", [KINDS[0], KINDS[2]], ids=["adam", "sgd-momentum"])
def test_two_runs_from_the_same_start_are_identical(gpu, kind):
    spans, total = _layout(SHAPES)
    lists = _pattern_lists(spans, "random", 8, 11)
    runs = []
    for _ in range(2):
        b = _buffers(kind, spans, total, 62, gpu)
        state = _new_state(gpu)
        for _ in range(2):
            _call(kind, b, spans, _dev_lists(lists, gpu), state, gpu)
        runs.append(b)
    _same(runs[0], runs[1])


@pytest.mark.parametrize("kind", [KINDS[0], KINDS[1]], ids=["adam", "sgd"])
def test_more_spans_and_lists_than_one_launch_takes(gpu, kind):
    """150 spans (a launch takes 64) and 70 lists (a launch takes 32): several launches, one counter advance, every
    span's union rows updated once."""
    shapes = [(3 + i % 5, 10 if i % 3 else 1) for i in range(150)]
    assert len(shapes) > 2 * SPANS_PER_LAUNCH
    spans, total = _layout(shapes)
    r = np.random.default_rng(17)
    lists = []
    for k in range(70):
        width = 10 if k % 2 else 1
        every = np.concatenate([off + width * np.arange(rows, dtype=np.int64) for off, rows, w in spans if w == width])
        d = r.permutation(every)[:40]
        lists.append((d, len(d), len(d), width))
    assert len(lists) > 2 * LISTS_PER_LAUNCH
    _, _, union = _check_call(kind, spans, total, lists, gpu)
    assert all(len(u) for u in union[:3]) and sum(len(u) for u in union) > 500
