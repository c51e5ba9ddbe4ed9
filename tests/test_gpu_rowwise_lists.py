"""GPU: the list-driven row-wise Adagrad step (include_dp/dfwfm_rowwise_lists.h), one process, no process group.

The call alone on a hand-built flat gradient buffer: spans (1, 10), (7, 10), (7, 1), (5000, 10), (5000, 1), (40, 2),
(40, 16), (40, 17), (40, 33) at 4-float-padded offsets, each with its own parameter, accumulator and stamp array;
W = 1, 2 and 8 lists per width, disjoint / identical / randomly overlapping lists, counts 0, 1, exactly cap and
cap + 5 over cap valid entries, the first and last row of the first and last span.  Expected: parameters and
accumulators of the union rows array_equal to dfwfm_rowwise_adagrad_row_ref (lib_rows) and to np_rows, untouched rows,
untouched accumulators and the pads bit-unchanged, touched gradient rows zero, the counter advanced by exactly one.
Then: the chain's order witnessed against a tree, the key-driven kernel on keys that touch the lists' union, the
global step and the scheduled entry over three calls, graph capture, run-to-run identity, more spans and lists than
one launch takes, and every error of the header's list."""
import ctypes

import numpy as np
import pytest
import torch

import rowwise_adagrad_ref as rw
import rowwise_lists_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
LR, WD, EPS = 1e-3, 3e-7, 1e-10
SHAPES = [(1, 10), (7, 10), (7, 1), (5000, 10), (5000, 1), (40, 2), (40, 16), (40, 17), (40, 33)]
WIDTHS = (10, 1, 2, 16, 17, 33)


def _stream(gpu):
    return ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


def _buffers(spans, total, seed, gpu):
    """Random tables, accumulators as after earlier steps (>= 0, every fourth one zero), a flat gradient (magnitudes
    1e-8 .. 1, the pads included), zero stamps."""
    r = np.random.default_rng(seed)
    b = {"p": [torch.from_numpy(r.standard_normal((rows, w)).astype(f32)).to(gpu) for _, rows, w in spans],
         "acc": [], "stamp": [torch.zeros(rows, dtype=torch.int32, device=gpu) for _, rows, _ in spans]}
    for _, rows, _ in spans:
        a = np.abs(0.1 * r.standard_normal(rows)).astype(f32)
        a[::4] = 0
        b["acc"].append(torch.from_numpy(a).to(gpu))
    g = (r.standard_normal(total) * 10.0 ** r.uniform(-8, 0, total)).astype(f32)
    b["g"] = torch.from_numpy(g).to(gpu)
    return b


def _host(b):
    return {k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in b.items()}


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


def _descriptors(b, spans, dl):
    from xsdeepfwfm_deprecated_amd import _lib
    sa = (_lib.dfwfm_rowwise_lists_span * max(len(spans), 1))()
    for i, (off, rows, w) in enumerate(spans):
        sa[i] = _lib.dfwfm_rowwise_lists_span(b["p"][i].data_ptr(), b["acc"][i].data_ptr(), b["stamp"][i].data_ptr(),
                                              off, rows, w, 0)
    la = (_lib.dfwfm_lazy_lists_list * max(len(dl), 1))()
    for i, (dest, count, cap, w) in enumerate(dl):
        la[i] = _lib.dfwfm_lazy_lists_list(dest.data_ptr(), count.data_ptr(), cap, w, 0)
    return sa, la


def _call(b, spans, dl, state, gpu, wd=WD, lr=LR, eps=EPS, sched=None):
    from xsdeepfwfm_deprecated_amd import _lib
    L, P = _lib.lib(), ctypes.c_void_p
    sa, la = _descriptors(b, spans, dl)
    h = rw.hyper(lr, wd, eps)
    g, st = P(b["g"].data_ptr()), P(state.data_ptr())
    if sched is not None:
        _lib.check(L.dfwfm_rowwise_adagrad_lists_step_dev_sched(sa, len(spans), la, len(dl), g, ctypes.byref(h),
                                                                P(sched.data_ptr()), st, _stream(gpu)), "lists")
    else:
        _lib.check(L.dfwfm_rowwise_adagrad_lists_step_dev(sa, len(spans), la, len(dl), g, ctypes.byref(h), st,
                                                          _stream(gpu)), "lists")


def _same(got, want, what=""):
    got, want = _host(got) if torch.is_tensor(got["g"]) else got, _host(want) if torch.is_tensor(want["g"]) else want
    assert np.array_equal(got["g"], want["g"]), (what, "g")
    for k in ("p", "acc"):
        for i, (a, c) in enumerate(zip(got[k], want[k])):
            assert np.array_equal(a, c, equal_nan=True), (what, k, i)


def _check_call(spans, total, lists, gpu, seed=3, step_before=0, wd=WD, eps=EPS):
    """One call from random buffers against the host function on the union rows (and against np_rows), with everything
    around it.  Returns the buffers after the call, those before it (host) and the union."""
    b = _buffers(spans, total, seed, gpu)
    before = _host(b)
    state = _new_state(gpu, step_before)
    _call(b, spans, _dev_lists(lists, gpu), state, gpu, wd=wd, eps=eps)
    torch.cuda.synchronize()
    assert int(state[0].item()) == step_before + 1 and int(state.view(torch.int32)[9].item()) == 0  # counter, ticket
    got = _host(b)
    for elem in ("lib", "np"):
        wp, wg, wa, union = ref.rowwise_lists_ref(before["p"], before["g"], before["acc"], spans, lists, lr=LR,
                                                  weight_decay=wd, eps=eps, elem=elem)
        _same(got, {"p": wp, "g": wg, "acc": wa}, elem)
    keep = np.ones(total, bool)
    for i, (span, touched) in enumerate(zip(spans, union)):
        rest = np.setdiff1d(np.arange(span[1]), touched)
        assert np.array_equal(got["p"][i][rest], before["p"][i][rest])  # every bit kept
        assert np.array_equal(got["acc"][i][rest], before["acc"][i][rest])
        assert not ref.grad_rows(got["g"], span)[touched].any()
        assert np.array_equal(np.flatnonzero(got["stamp"][i]), touched)  # claimed exactly the union
        ref.grad_rows(keep, span)[touched] = False
    assert np.array_equal(got["g"][keep], before["g"][keep])  # untouched gradient rows and the pads
    return b, before, union


def _pool(spans, width, n, seed):
    """Up to n distinct destinations of rows in the spans of `width`: always the first and the last row of every such
    span (so of the first and of the last span of all), the rest random."""
    r = np.random.default_rng(seed)
    mine = [(off, rows) for off, rows, w in spans if w == width]
    forced = np.fromiter(sorted({d for off, rows in mine for d in (off, off + (rows - 1) * width)}), np.int64)
    every = np.concatenate([off + width * np.arange(rows, dtype=np.int64) for off, rows in mine])
    rest = np.setdiff1d(every, forced)
    take = r.permutation(rest)[:max(0, min(n, len(every)) - len(forced))]
    return r.permutation(np.concatenate([forced, take])), np.setdiff1d(rest, take), forced


def _pattern_lists(spans, pattern, W, seed, widths=WIDTHS):
    """W lists per width.  Behind each list's count sit `spare` destinations of rows no list names (they must stay
    untouched: the reader stops at the count)."""
    lists = []
    for width in widths:
        pool, spare, forced = _pool(spans, width, 330 if width in (10, 1) else 30, seed + width)
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
@pytest.mark.parametrize("wd", [0.0, WD])
@pytest.mark.parametrize("pattern", ["disjoint", "same", "random"])
@pytest.mark.parametrize("W", [1, 2, 8])
def test_lists_call_equals_the_host_function_on_union_rows(gpu, W, pattern, wd):
    """The nine spans, W lists per width (6 W lists): every tensor bit for bit against dfwfm_rowwise_adagrad_row_ref
    and np_rows on the union rows; the first and last row of the first and last span are listed."""
    spans, total = ref.layout(SHAPES)
    lists = _pattern_lists(spans, pattern, W, 40 + W)
    _, _, union = _check_call(spans, total, lists, gpu, step_before=1, wd=wd)
    assert union[0].tolist() == [0] and {0, 6} <= set(union[2].tolist()) and {0, 39} <= set(union[8].tolist())
    assert {0, 4999} <= set(union[3].tolist()) and {0, 4999} <= set(union[4].tolist())
    assert sum(len(u) for u in union) > 300 and all(len(u) for u in union)
    if pattern == "same" and W > 1:  # every row named W times, updated once
        assert sum(len(u) for u in union) * W == sum(c for _, c, _, _ in lists)


def test_counts_zero_one_cap_and_past_cap(gpu):
    """Per width five lists: count 0 (its entries must not be read), 1, exactly cap, and cap + 5 over cap valid entries
    (the reader stops at cap); a negative count reads nothing."""
    spans, total = ref.layout(SHAPES)
    lists = []
    for width in WIDTHS:
        pool = _pool(spans, width, 40, 5 + width)[0]
        lists += [(pool[0:6], 0, 6, width), (pool[6:12], 1, 6, width), (pool[12:20], 8, 8, width),
                  (pool[20:31], 16, 11, width), (pool[31:35], -2, 4, width)]
    _, _, union = _check_call(spans, total, lists, gpu, step_before=1)
    assert sum(len(u) for u in union) == len(WIDTHS) * (1 + 8 + 11)


def test_zero_accumulators_and_the_default_eps(gpu):
    """Accumulators all zero (a first step) with eps 1e-10, and a touched row whose gradient is exactly zero: it is
    still updated by the weight decay alone."""
    spans, total = ref.layout(SHAPES)
    lists = _pattern_lists(spans, "random", 2, 12)
    b = _buffers(spans, total, 9, gpu)
    for a in b["acc"]:
        a.zero_()
    ref.grad_rows(b["g"], spans[1])[0] = 0.0  # row 0 of the (7, 10) span is in every pool
    before = _host(b)
    state = _new_state(gpu)
    _call(b, spans, _dev_lists(lists, gpu), state, gpu)
    wp, wg, wa, union = ref.rowwise_lists_ref(before["p"], before["g"], before["acc"], spans, lists, lr=LR,
                                              weight_decay=WD, eps=EPS, elem="lib")
    _same(b, {"p": wp, "g": wg, "acc": wa})
    assert 0 in union[1] and not np.array_equal(wp[1][0], before["p"][1][0]) and wa[1][0] > 0
    assert not np.isnan(np.concatenate([p.reshape(-1) for p in wp])).any()


def test_empty_lists_advance_the_counter_only(gpu):
    """All counts zero, no list, no span: nothing changes and the counter advances by exactly one per call."""
    spans, total = ref.layout(SHAPES)
    b = _buffers(spans, total, 8, gpu)
    want = _host(b)
    state = _new_state(gpu)
    pool = _pool(spans, 10, 12, 1)[0]
    _call(b, spans, _dev_lists([(pool, 0, len(pool), 10), (pool, 0, len(pool), 10)], gpu), state, gpu)
    assert int(state[0].item()) == 1
    _call(b, spans, [], state, gpu)
    assert int(state[0].item()) == 2
    _call(b, [], [], state, gpu)  # n_spans == 0
    torch.cuda.synchronize()
    assert int(state[0].item()) == 3 and int(state.view(torch.int32)[9].item()) == 0
    _same(b, want)
    assert not any(s.any().item() for s in b["stamp"])


def test_destinations_in_no_span_are_skipped(gpu):
    """Destinations in a pad, between two rows, in a span of another width, below the first span's offset, past the
    last span and negative: not written, not an error, and the bits beside them are unchanged (the whole of every
    buffer is compared); the valid ones beside them are updated."""
    spans, total = ref.layout(SHAPES)
    spans = [(off + 16, rows, w) for off, rows, w in spans]  # nothing at floats 0 .. 15
    total += 16
    o = [s[0] for s in spans]
    lists = [(np.array([o[1] + 20, o[0] + 10, o[1] + 5, o[2], 0, 8, total, 2 ** 40, -10, o[3] + 49990, o[6]], np.int64),
              11, 11, 10),                                            # o[1] + 5: between rows; o[2], o[6]: other widths
             (np.array([o[2] + 3, o[2] + 7, o[1], o[4] + 5000, -1, o[4], o[5] + 1], np.int64), 7, 7, 1),
             (np.array([o[6] + 16, o[7] + 16, o[6] + 8, o[7], total + 16], np.int64), 5, 5, 16),  # o[7]: width 17
             (np.array([o[7] + 17 * 39, o[6] + 17, o[7] + 16, o[8]], np.int64), 4, 4, 17),
             (np.array([o[8] + 33, o[8] + 34, o[8] + 33 * 40, o[7] + 33], np.int64), 4, 4, 33)]  # o[8] + 33 * 40: the end
    _, _, union = _check_call(spans, total, lists, gpu)
    assert [u.tolist() for u in union] == [[], [2], [3], [4999], [0], [], [1], [39], [1]]


def test_the_order_of_the_chain_is_witnessed(gpu):
    """On this test's data a pairwise tree of the same squares gives other bits than the chain on at least one touched
    row (asserted first: the order is witnessed, not assumed); the kernel gives the chain's."""
    spans, total = ref.layout(SHAPES)
    lists = _pattern_lists(spans, "random", 2, 42)
    before = _host(_buffers(spans, total, 3, gpu))
    chain = ref.rowwise_lists_ref(before["p"], before["g"], before["acc"], spans, lists, lr=LR, weight_decay=WD)
    tree = ref.rowwise_lists_ref(before["p"], before["g"], before["acc"], spans, lists, lr=LR, weight_decay=WD,
                                 ss_of=rw.tree_ss)
    differ = [i for i in range(len(spans)) if not np.array_equal(chain[2][i], tree[2][i])]
    assert differ and all(spans[i][2] > 1 for i in differ)  # (one square has one order only)
    assert any(not np.array_equal(chain[0][i], tree[0][i]) for i in differ)
    b, _, _ = _check_call(spans, total, lists, gpu)  # seed 3 as above: equal to the chain, hence not the tree
    got = _host(b)
    for i in differ:
        assert np.array_equal(got["acc"][i], chain[2][i]) and not np.array_equal(got["acc"][i], tree[2][i])


def test_key_driven_kernel_gives_the_same_bits_on_keys_that_touch_the_union(gpu):
    """dfwfm_rowwise_adagrad_step_dev on the same tables, with keys that touch exactly the lists' union: the same bits
    in param, state and grad -- the two kernels share one copy of the row's arithmetic."""
    from xsdeepfwfm_deprecated_amd import _lib
    spans, total = ref.layout(SHAPES)
    lists = _pattern_lists(spans, "random", 2, 42)
    a, _, union = _check_call(spans, total, lists, gpu)
    c = _buffers(spans, total, 3, gpu)
    keys, index = ref.keys_for(union)
    assert index == list(range(len(spans)))
    xi = torch.from_numpy(keys).to(gpu)
    tabs = (_lib.dfwfm_rowwise_table * len(index))()
    for j, i in enumerate(index):
        off, rows, w = spans[i]
        tabs[j] = _lib.dfwfm_rowwise_table(c["p"][i].data_ptr(), c["g"][off:].data_ptr(), c["acc"][i].data_ptr(),
                                           c["stamp"][i].data_ptr(), rows, rows, 0, w, j, _lib.LAZY_PLAIN, 0)
    state = _new_state(gpu)
    h = rw.hyper(LR, WD, EPS)
    _lib.check(_lib.lib().dfwfm_rowwise_adagrad_step_dev(tabs, len(index), ctypes.c_void_p(xi.data_ptr()), xi.stride(0),
                                                         xi.shape[0], ctypes.byref(h),
                                                         ctypes.c_void_p(state.data_ptr()), _stream(gpu)), "keys")
    torch.cuda.synchronize()
    _same(a, c)
    assert int(state[0].item()) == 1


def test_three_calls_use_the_global_step_and_the_schedule(gpu):
    """Three calls with a schedule: at every step the scheduled entry gives the bits of the unscheduled entry with
    lr = dfwfm_lr_schedule_eval(step), and of the host function at that rate.  Row 3 of the (7, 10) span is listed at
    steps 1 and 3 only: it keeps its bits at step 2."""
    from xsdeepfwfm_deprecated_amd import _lib
    spans, total = ref.layout(SHAPES)
    knots = [(1, 1e-4), (3, 1e-3)]
    sched = torch.zeros(_lib.LR_SCHEDULE_BYTES // 8, dtype=torch.int64, device=gpu)
    arr, n = _lib.lr_knots(knots)
    _lib.check(_lib.lib().dfwfm_lr_schedule_write(ctypes.c_void_p(sched.data_ptr()), arr, n, _stream(gpu)), "write")
    o = spans[1][0]
    extra = [[(np.array([o + 30, o + 50], np.int64), 2, 2, 10)],
             [(np.array([o + 10, o + 50], np.int64), 2, 2, 10)],
             [(np.array([o + 30], np.int64), 1, 1, 10), (np.array([o + 30, o], np.int64), 2, 2, 10)]]
    a, c = _buffers(spans, total, 21, gpu), _buffers(spans, total, 21, gpu)
    want = _host(a)
    sa, sc = _new_state(gpu), _new_state(gpu)
    row3, rates = [], set()
    for s, lists in enumerate(extra, 1):
        lists = lists + _pattern_lists(spans, "random", 1, 50 + s, widths=(1, 17, 33))
        lr = _lib.lr_schedule_eval(knots, s)
        rates.add(lr)
        g = _buffers(spans, total, 30 + s, gpu)["g"]
        a["g"].copy_(g)
        c["g"].copy_(g)
        _call(a, spans, _dev_lists(lists, gpu), sa, gpu, lr=123.0, sched=sched)  # lr unused
        _call(c, spans, _dev_lists(lists, gpu), sc, gpu, lr=lr)
        _same(a, c, s)
        wp, wg, wa, _ = ref.rowwise_lists_ref(want["p"], g.cpu().numpy(), want["acc"], spans, lists, lr=lr,
                                              weight_decay=WD, eps=EPS, elem="lib")
        want = {"p": wp, "g": wg, "acc": wa}
        _same(a, want, s)
        assert int(sa[0].item()) == int(sc[0].item()) == s
        row3.append(a["p"][1][3].cpu().numpy().copy())
    assert len(rates) == 3
    assert np.array_equal(row3[0], row3[1]) and not np.array_equal(row3[1], row3[2])


def test_captured_call_replayed_three_times_equals_three_eager_calls(gpu):
    """One captured call, replayed with new destinations, counts and gradients written into the same buffers between
    replays: counts, destinations, gradients and the counter are read afresh."""
    spans, total = ref.layout(SHAPES)
    steps = [_pattern_lists(spans, p, 2, 90 + i) for i, p in enumerate(("random", "disjoint", "same"))]
    cap = {w: max(l[2] for ls in steps for l in ls if l[3] == w) for w in WIDTHS}
    dl = [(torch.zeros(cap[w], dtype=torch.int64, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu), cap[w], w)
          for _, _, _, w in steps[0]]
    grads = [_buffers(spans, total, 100 + s, gpu)["g"] for s in range(3)]

    def load(lists):
        for (dest, count, _, _), (d, c, _, _) in zip(dl, lists):
            dest[:len(d)].copy_(torch.from_numpy(np.asarray(d, np.int64).copy()))
            count.fill_(c)

    a, c = _buffers(spans, total, 61, gpu), _buffers(spans, total, 61, gpu)
    sa, sc = _new_state(gpu), _new_state(gpu)
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    load(steps[0])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            _call(a, spans, dl, sa, gpu)
    torch.cuda.current_stream(gpu).wait_stream(s)
    assert int(sa[0].item()) == 0  # captured, not run
    for lists, g in zip(steps, grads):
        load(lists)
        a["g"].copy_(g)
        graph.replay()
        c["g"].copy_(g)
        _call(c, spans, _dev_lists(lists, gpu), sc, gpu)
    torch.cuda.synchronize()
    _same(a, c)
    assert int(sa[0].item()) == int(sc[0].item()) == 3


def test_two_runs_from_the_same_start_are_identical(gpu):
    spans, total = ref.layout(SHAPES)
    lists = _pattern_lists(spans, "random", 8, 11)
    runs = []
    for _ in range(2):
        b = _buffers(spans, total, 62, gpu)
        state = _new_state(gpu)
        for _ in range(2):
            b["g"].copy_(_buffers(spans, total, 63, gpu)["g"])
            _call(b, spans, _dev_lists(lists, gpu), state, gpu)
        runs.append(b)
    _same(runs[0], runs[1])


def test_more_spans_and_lists_than_one_launch_takes(gpu):
    """150 spans and 70 lists, more than two launches' worth of each: several launches, one counter advance, every
    span's union rows updated once."""
    from xsdeepfwfm_deprecated_amd import _lib
    shapes = [(3 + i % 5, (10, 1, 17)[i % 3]) for i in range(150)]
    assert len(shapes) > 2 * _lib.ROWWISE_LISTS_SPANS_PER_LAUNCH
    spans, total = ref.layout(shapes)
    r = np.random.default_rng(17)
    lists = []
    for k in range(70):
        width = (10, 1, 17)[k % 3]
        every = np.concatenate([off + width * np.arange(rows, dtype=np.int64) for off, rows, w in spans if w == width])
        d = r.permutation(every)[:40]
        lists.append((d, len(d), len(d), width))
    assert len(lists) > 2 * _lib.ROWWISE_LISTS_LISTS_PER_LAUNCH
    _, _, union = _check_call(spans, total, lists, gpu)
    assert all(len(u) for u in union[:3]) and sum(len(u) for u in union) > 400


# ------------------------------------------------------------------------------------------------ the errors
def test_every_error_returns_invalid_arg_with_no_launch(gpu):
    """Every line of the header's list on real device buffers: DFWFM_ERR_INVALID_ARG (the too-long list:
    DFWFM_ERR_UNSUPPORTED), a message, and no launch -- the counter and every buffer are unchanged."""
    from xsdeepfwfm_deprecated_amd import _lib
    import optim_ref
    L, P = _lib.lib(), ctypes.c_void_p
    spans, total = ref.layout(SHAPES[:3])
    b = _buffers(spans, total, 4, gpu)
    want = _host(b)
    state = _new_state(gpu, 5)
    sched = torch.zeros(_lib.LR_SCHEDULE_BYTES // 8, dtype=torch.int64, device=gpu)
    arr, n = _lib.lr_knots([(1, LR)])
    _lib.check(L.dfwfm_lr_schedule_write(P(sched.data_ptr()), arr, n, _stream(gpu)), "write")
    dl = _dev_lists([(np.array([spans[1][0], spans[1][0] + 10], np.int64), 2, 2, 10),
                     (np.array([spans[2][0]], np.int64), 1, 1, 1)], gpu)
    good = rw.hyper(LR, WD, EPS)
    nan, inf = float("nan"), float("inf")

    def refused(word, rc=-1, span=None, lst=None, only=None, grad=True, st=True, block=True, h=good, ns=None, nl=None,
                null_spans=False, null_lists=False):
        sa, la = _descriptors(b, spans, dl)
        for i, kw in (span or {}).items():
            for k, v in kw.items():
                setattr(sa[i], k, v)
        for i, kw in (lst or {}).items():
            for k, v in kw.items():
                setattr(la[i], k, v)
        sa_, la_ = (None if null_spans else sa), (None if null_lists else la)
        ns_, nl_ = (len(spans) if ns is None else ns), (len(dl) if nl is None else nl)
        g = P(b["g"].data_ptr()) if grad else None
        s = P(state.data_ptr()) if st else None
        hp = None if h is None else ctypes.byref(h)
        calls = [("dev", lambda: L.dfwfm_rowwise_adagrad_lists_step_dev(sa_, ns_, la_, nl_, g, hp, s, _stream(gpu))),
                 ("sched", lambda: L.dfwfm_rowwise_adagrad_lists_step_dev_sched(
                     sa_, ns_, la_, nl_, g, hp, P(sched.data_ptr()) if block else None, s, _stream(gpu)))]
        for name, call in calls:
            if only is None or name in only:
                assert call() == rc, (name, word)
                assert word in L.dfwfm_last_error(), (name, word, L.dfwfm_last_error())

    # the hyper-parameters
    refused(b"null hyper", h=None)
    for kind in ("sgd", "rmsp"):
        refused(b"not DFWFM_OPTIM_ADAGRAD", h=optim_ref.hyper(kind, LR))
    refused(b"unknown optimizer kind", h=optim_ref.hyper(7, LR))
    for field in ("lr", "weight_decay", "momentum", "alpha", "eps"):
        for bad in (nan, inf, -1e-9):
            h = rw.hyper(LR, WD, EPS)
            setattr(h, field, bad)
            refused(field.encode(), h=h, only=("dev",) if field == "lr" else None)
    h = rw.hyper(LR)
    h.alpha = 1.0
    refused(b"alpha", h=h)
    # the blocks and the arrays
    refused(b"null state block", st=False)
    refused(b"null schedule", block=False, only=("sched",))
    refused(b"null grad", grad=False)
    refused(b"null span array", null_spans=True)
    refused(b"null list array", null_lists=True)
    refused(b"negative span count", ns=-1)
    refused(b"negative list count", nl=-1)
    # per span
    refused(b"null pointer", span={1: dict(param=None)})
    refused(b"null state pointer", span={1: dict(state=None)})
    refused(b"null pointer", span={2: dict(stamp=None)})
    refused(b"rows", span={0: dict(rows=0)})
    refused(b"width", span={0: dict(width=0)})
    refused(b"negative offset", span={0: dict(offset=-4)})
    refused(b"overlapping", span={2: dict(offset=spans[1][0] + 69)})
    refused(b"63 bits", span={1: dict(offset=2 ** 62, rows=2 ** 60)})  # (width 10: 2^62 + 10 * 2^60 is past 2^63)
    # per list
    refused(b"cap < 0", lst={0: dict(cap=-1)})
    refused(b"null pointer", lst={1: dict(dest=None)})
    refused(b"null pointer", lst={1: dict(count=None)})
    refused(b"matches no span", lst={0: dict(width=0)})
    refused(b"matches no span", lst={0: dict(width=16)})
    refused(b"matches no span", ns=0)
    refused(b"too long", rc=-2, lst={0: dict(cap=256 * (2 ** 30 + 1))})
    torch.cuda.synchronize()
    assert int(state[0].item()) == 5 and int(state.view(torch.int32)[9].item()) == 0
    _same(b, want)
    assert not any(s.any().item() for s in b["stamp"])
    _call(b, spans, dl, state, gpu)  # and the same descriptors, unspoilt, run
    assert int(state[0].item()) == 6 and sum(int(s.count_nonzero().item()) for s in b["stamp"]) == 3
