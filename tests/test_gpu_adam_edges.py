"""GPU: the Adam kernels (adam_kernel through dfwfm_adam_step, adam_dev_kernel through dfwfm_adam_step_dev) at their
edges; fixtures and references in tests/dense_edge_cases.py, the CPU leg in tests/test_dense_edge_cases.py.

1. csrc/dfwfm_adam.h's promise for dfwfm_adam_step: one element gets the same bits wherever it sits -- at any place
   of a tensor of any length (the float4 body, the last numel % 4 elements), with any of its four arrays off the
   16-byte grid (the element-wise path), and as any tensor of a list that takes three launches (kAdamList = 91) with
   null-grad and empty entries between (the binary search over block0) -- and writes nothing around its tensors.
2. dfwfm_adam_step_dev against dfwfm_adam_step at the same step number: the same bits but for the last numel % 4
   elements (one rounding of v apart, and equal where v was 0); its device counter advances once per call, however
   many launches the call makes, the ticket returns to 0 and the stored scalars are the step's; more blocks than the
   grid (kAdamGrid = 2048) are walked.
3. Steps 1 .. 2^31, betas down to beta1 = 0 (where torch's lerp takes its other form), weight decay and eps (0
   included) against a float64 restatement of torch's single-tensor Adam and against torch.optim.Adam on the CPU.
4. Gradients that are 0, underflow when squared, leave v subnormal, overflow when squared, NaN and +-inf, each beside
   ordinary neighbours in one float4: torch's class element for element, and the neighbours' bits unchanged.

Worst figures measured on an MI355X (each test prints its own; run with -s), the same for dfwfm_adam_step and
dfwfm_adam_step_dev and for every step number; p as a fraction of its bar (rtol 2.4e-7, atol 2e-9), exp_avg and
exp_avg_sq as relative error against float64 (bar 2.4e-7).  Evidence of margin, not thresholds.

    betas           p against float64 / torch CPU     exp_avg     exp_avg_sq    (torch float32 itself: CPU leg)
    (0.9, 0.999)    0.25 / 0.47                       6.4e-8      7.2e-8        (6.4e-8, 1.2e-7)
    (0.5, 0.9)      0.25 / 0.48                       9.9e-8      8.5e-8        (9.9e-8, 1.2e-7)
    (0.3, 0.999)    0.25 / 0.45                       1.0e-7      7.2e-8        (1.0e-7, 1.2e-7)
    (0.0, 0.5)      0.25 / 0.46                       9.2e-8      1.6e-7        (9.2e-8, 1.6e-7)

adam_dev_kernel against adam_kernel over the 0 / 1 / 91 / 92 / 183-tensor calls: 94 of the tail elements differ, each
by one rounding of v; none with v = 0 on entry.

With the kernels broken on purpose (wrong values only) these tests failed: adam_kernel with kAdamFuseG on its
element-wise paths (numel, alignment, list position); adam_block without its tail loop (the `plain` fixture those
three share, the grid walk, every step / betas case); dfwfm_adam_step_dev bumping the counter only on a
single-launch call (the 92- and 183-tensor calls of test_adam_dev_matches_host_and_counts_once_per_call).
"""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import dense_edge_cases as dc

pytestmark = pytest.mark.gpu

GUARD = np.float32(-12345.5)
HYPER = (dc.ADAM_LR, 0.9, 0.999, 1e-8, dc.L2)  # lr, beta1, beta2, eps, weight_decay
STEP = 3


class Flat:
    """One flat float32 buffer holding every array of a tensor list, GUARD floats around each: add() places an array
    at a 16-byte aligned offset plus `mis` floats; run() uploads, calls the kernel, downloads and checks the guards."""

    def __init__(self):
        self.size, self.chunks, self.entries = 8, [], []

    def add(self, arr, mis=0):
        off = (self.size + 3) // 4 * 4 + mis
        self.chunks.append((off, np.asarray(arr, np.float32)))
        self.size = off + len(arr) + 8
        return off

    def tensor(self, p, g, m, v, mis=(0, 0, 0, 0), live=True):
        """Appends a list entry; g None: a null grad.  Returns the entry's index."""
        offs = [self.add(a, k) for a, k in zip((p, g if g is not None else [], m, v), mis)]
        self.entries.append((offs, len(p), g is not None))
        return len(self.entries) - 1

    def run(self, gpu, call):
        from xsdeepfwfm_deprecated_amd import _lib
        host = np.full(self.size + 8, GUARD, np.float32)
        used = np.zeros(len(host), bool)
        for off, a in self.chunks:
            host[off:off + len(a)] = a
            used[off:off + len(a)] = True
        dev = torch.from_numpy(host).to(gpu)
        base = dev.data_ptr()
        assert base % 16 == 0
        arr = (_lib.dfwfm_adam_tensor * max(len(self.entries), 1))()
        for i, ((op, og, om, ov), n, has_g) in enumerate(self.entries):
            arr[i] = _lib.dfwfm_adam_tensor(base + 4 * op, base + 4 * og if has_g else None, base + 4 * om,
                                            base + 4 * ov, n)
        call(arr, len(self.entries))
        torch.cuda.synchronize()
        self.out = dev.cpu().numpy()
        assert np.all(self.out[~used] == GUARD), "a guard float was written"
        for (op, og, om, ov), n, has_g in self.entries:  # gradients are read only
            if has_g:
                assert np.array_equal(self.out[og:og + n].view(np.int32), host[og:og + n].view(np.int32))
        return self

    def result(self, i):
        (op, _, om, ov), n, _ = self.entries[i]
        return self.out[op:op + n], self.out[om:om + n], self.out[ov:ov + n]


def _stream(gpu):
    return ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


def host_call(gpu, hyper=HYPER, step=STEP):
    """dfwfm_adam_step, as engine.adam_step calls it."""
    from xsdeepfwfm_deprecated_amd import _lib
    lr, b1, b2, eps, wd = hyper
    return lambda arr, n: _lib.check(_lib.lib().dfwfm_adam_step(arr, n, float(lr), float(b1), float(b2), float(eps),
                                                                float(wd), int(step), _stream(gpu)), "adam")


def dev_call(gpu, state, hyper=HYPER):
    from xsdeepfwfm_deprecated_amd import _lib
    lr, b1, b2, eps, wd = hyper
    return lambda arr, n: _lib.check(_lib.lib().dfwfm_adam_step_dev(arr, n, float(lr), float(b1), float(b2),
                                                                    float(eps), float(wd),
                                                                    ctypes.c_void_p(state.data_ptr()), _stream(gpu)),
                                     "adam dev")


def new_state(gpu, step_before=0):
    """The zeroed 48-byte state block with its int64 counter (the first 8 bytes) preset."""
    from xsdeepfwfm_deprecated_amd import _lib
    assert _lib.ADAM_STATE_BYTES == dc.ADAM_STATE_BYTES
    st = torch.zeros(dc.ADAM_STATE_BYTES // 8, dtype=torch.int64, device=gpu)
    st[0] = step_before
    return st


def read_state(state):
    """(step, (step_size, omb1, b2, omb2, eps, wd, bc2_sqrt), ticket) of AdamDevState."""
    raw = state.cpu().numpy().tobytes()
    step, = struct.unpack_from("<q", raw, 0)
    scal = np.frombuffer(raw, np.float32, 7, 8)
    ticket, = struct.unpack_from("<i", raw, 36)
    return step, scal, ticket


def step_scalars(step, hyper):
    """dfwfm_adam.h adam_coef: the step's scalars from doubles, rounded to float32 per use."""
    lr, b1, b2, eps, wd = hyper
    bc1, bc2 = 1.0 - math.pow(b1, step), 1.0 - math.pow(b2, step)
    return np.asarray([lr / bc1, 1.0 - b1, b2, 1.0 - b2, eps, wd, math.sqrt(bc2)], np.float64).astype(np.float32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


@pytest.fixture(scope="module")
def plain(gpu):
    """The value vector's update as one aligned tensor through dfwfm_adam_step: every other placement's reference."""
    vals = dc.adam_values()
    f = Flat()
    f.tensor(*vals)
    p, m, v = f.run(gpu, host_call(gpu)).result(0)
    r64 = dc.adam_ref64(*vals, STEP, *HYPER[:4], HYPER[4])
    assert dc.p_err(p, r64[0]) <= 1.0  # and it is Adam's update (part 3's bar on p; m and g + wd p cancel here)
    assert not same_bits(p, vals[0]) and not same_bits(m, vals[2]) and not same_bits(v, vals[3])
    return vals, (p.copy(), m.copy(), v.copy())


def _assert_prefix(f, i, n, want, what):
    for got, ref, name in zip(f.result(i), want, "pmv"):
        assert same_bits(got, ref[:n]), (what, name, int(np.flatnonzero(got != ref[:n])[0]))


# ---------------------------------------------------------------------------------------------------------- 1
def test_adam_bits_do_not_depend_on_numel(gpu, plain):
    vals, want = plain
    f = Flat()
    for n in dc.ADAM_NUMELS:
        f.tensor(*(a[:n] for a in vals))
    f.run(gpu, host_call(gpu))
    for i, n in enumerate(dc.ADAM_NUMELS):
        _assert_prefix(f, i, n, want, f"numel {n}")


@pytest.mark.parametrize("which", ["p", "g", "m", "v", "all"])
def test_adam_bits_do_not_depend_on_alignment(gpu, plain, which):
    """One array off the 16-byte grid selects the element-wise path for the whole tensor."""
    vals, want = plain
    f = Flat()
    for off in range(4):
        f.tensor(*vals, mis=tuple(off if which in (name, "all") else 0 for name in "pgmv"))
    f.run(gpu, host_call(gpu))
    for off in range(4):
        _assert_prefix(f, off, dc.ADAM_N, want, f"{which} at float offset {off}")


def _long_list(vals, v_zero=False):
    """183 live tensors -- the value vector at ADAM_SLOTS, prefixes of it of 1 .. 8193 elements elsewhere (several
    4096-element blocks in some: runs in block0) -- with a null-grad and an empty entry after every fifth.
    Returns (Flat, [(entry, numel)] of the live ones)."""
    rng = np.random.default_rng(183)
    sizes = rng.choice([1, 2, 3, 5, 7, 64, 255, 1023, 1024, 1025, 4095, 4096, 4097, 5000, 8192, 8193], dc.ADAM_LIVE)
    f, live = Flat(), []
    p, g, m, v = vals
    if v_zero:
        v = np.zeros_like(v)
    for k in range(dc.ADAM_LIVE):
        n = dc.ADAM_N if k in dc.ADAM_SLOTS else int(sizes[k])
        live.append((f.tensor(p[:n], g[:n], m[:n], v[:n]), n))
        if k % 5 == 4:
            f.tensor(p[:9], None, m[:9], v[:9])           # no grad: skipped, untouched
            f.tensor(p[:0], g[:0], m[:0], v[:0])          # numel 0
    return f, live


def test_adam_bits_do_not_depend_on_list_position(gpu, plain):
    vals, want = plain
    f, live = _long_list(vals)
    assert len(live) == 183 and len(f.entries) > 183
    f.run(gpu, host_call(gpu))
    for k, (i, n) in enumerate(live):
        _assert_prefix(f, i, n, want, f"tensor {k} of 183")
    for i, ((op, _, om, ov), n, has_g) in enumerate(f.entries):  # a null grad leaves p, m and v alone
        if not has_g:
            assert all(same_bits(a, b[:n]) for a, b in zip(f.result(i), (vals[0], vals[2], vals[3])))


# ---------------------------------------------------------------------------------------------------------- 2
def _assert_dev_equals_host(fd, fh, live, what):
    """adam_dev_kernel against adam_kernel: the same bits on the first numel - numel % 4 elements; the rest within one
    float32 rounding of v (m the same bits, p at part 3's bar).  Returns the number of tail elements that differ."""
    differ = 0
    for i, n in live:
        body = n - n % 4
        for d, h, name in zip(fd.result(i), fh.result(i), "pmv"):
            assert same_bits(d[:body], h[:body]), (what, i, name)
        (dp, dm, dv), (hp, hm, hv) = fd.result(i), fh.result(i)
        assert same_bits(dm[body:], hm[body:]), (what, i)
        assert np.all(np.abs(dv[body:].astype(np.float64) - hv[body:]) <= np.spacing(np.abs(hv[body:]))), (what, i)
        assert dc.p_err(dp[body:], hp[body:]) <= 1.0, (what, i)
        differ += int(np.count_nonzero(dv[body:] != hv[body:]))
    return differ


@pytest.mark.parametrize("v_zero", [False, True], ids=["v", "v0"])
def test_adam_dev_matches_host_and_counts_once_per_call(gpu, v_zero):
    """Calls of 0, 1, 91, 92 and 183 tensors (one launch, the launch boundary, three launches) on one state block,
    from step 7 on: after each the counter is one higher, the ticket 0 and the scalars that step's."""
    vals = dc.adam_values()
    full, live_all = _long_list(vals, v_zero)
    step = 7
    state = new_state(gpu, step - 1)
    differ = 0
    for count in (0, 1, 91, 92, 183):
        fd, fh = (_long_list(vals, v_zero)[0] for _ in range(2))
        keep = live_all[count - 1][0] + 1 if count else 0  # the entries up to the count-th live tensor
        for f in (fd, fh):
            f.entries = f.entries[:keep]
        fd.run(gpu, dev_call(gpu, state))
        fh.run(gpu, host_call(gpu, step=step))
        got_step, scal, ticket = read_state(state)
        assert got_step == step and ticket == 0, (count, got_step, ticket)
        assert same_bits(scal, step_scalars(step, HYPER)), (count, scal)
        d = _assert_dev_equals_host(fd, fh, live_all[:count], f"{count} tensors")
        assert not (v_zero and d), "v = 0 on entry: the two forms of the second moment's sum agree"
        differ += d
        step += 1
    print(f"adam_dev against adam_kernel, v {'= 0' if v_zero else '!= 0'}: {differ} tail elements one rounding apart")


def test_adam_dev_walks_more_blocks_than_its_grid(gpu):
    """2048 x 4096 + 4097 elements: 2050 blocks on a grid of 2048, then a 5-element tensor (a float4 and a tail)."""
    from xsdeepfwfm_deprecated_amd import _lib
    n_big = dc.ADAM_GRID * dc.ADAM_BLOCK + 4097
    gen = torch.Generator(device=gpu).manual_seed(5)
    sizes = (n_big, 5)
    init = []
    for n in sizes:
        p = torch.randn(n, device=gpu, generator=gen)
        g = torch.randn(n, device=gpu, generator=gen) * 1e-2
        m = g * 0.5
        v = g * g * 0.75 + 1e-12
        init.append((p, g, m, v))
    res = []
    state = new_state(gpu, STEP - 1)
    for call in (dev_call(gpu, state), host_call(gpu)):
        ts = [tuple(a.clone() for a in t) for t in init]
        arr = (_lib.dfwfm_adam_tensor * len(ts))(*[_lib.dfwfm_adam_tensor(p.data_ptr(), g.data_ptr(), m.data_ptr(),
                                                                         v.data_ptr(), p.numel())
                                                   for p, g, m, v in ts])
        assert all(a.data_ptr() % 16 == 0 for t in ts for a in t)
        call(arr, len(ts))
        torch.cuda.synchronize()
        res.append(ts)
    got_step, scal, ticket = read_state(state)
    assert got_step == STEP and ticket == 0 and same_bits(scal, step_scalars(STEP, HYPER))
    for (dp, dg, dm, dv), (hp, hg, hm, hv), (ip, ig, im, iv) in zip(res[0], res[1], init):
        n = dp.numel()
        body = n - n % 4
        for d, h, i in ((dp, hp, ip), (dm, hm, im), (dv, hv, iv)):
            assert torch.equal(d[:body].view(torch.int32), h[:body].view(torch.int32))
            assert not torch.equal(d.view(torch.int32), i.view(torch.int32))
        # every block was visited: no element of m kept its old value (m' = m + 0.1 (g - m) != m for g != m)
        assert int((dm == im).sum().item()) <= int((ig == im).sum().item())
        assert torch.equal(dg, ig)
        tail = slice(body, n)
        assert torch.equal(dm[tail], hm[tail])
        assert bool(((dv[tail].double() - hv[tail].double()).abs() <= 2.0 ** -23 * hv[tail].double()).all())
        assert dc.p_err(dp[tail].cpu().numpy(), hp[tail].cpu().numpy()) <= 1.0


# ---------------------------------------------------------------------------------------------------------- 3
def _grid_case(gpu, api, step, betas, wd, eps, gmin):
    vals, r64, t32 = dc.adam_grid_case(step, betas, wd, eps, gmin)
    hyper = (dc.ADAM_LR, betas[0], betas[1], eps, wd)
    f = Flat()
    f.tensor(*vals)
    if api == "host":
        f.run(gpu, host_call(gpu, hyper, step))
    else:
        state = new_state(gpu, step - 1)
        f.run(gpu, dev_call(gpu, state, hyper))
        assert read_state(state)[0] == step
    p, m, v = f.result(0)
    e = (dc.p_err(p, r64[0]), dc.rel_err(m, r64[1]), dc.rel_err(v, r64[2]), dc.p_err(p, t32[0]))
    rt = dc.MV_RTOL[betas]
    assert e[0] <= 1.0 and e[1] <= rt and e[2] <= rt, (step, betas, wd, eps, e)
    assert e[3] <= 1.0, (step, betas, wd, eps, e)  # torch.optim.Adam on the CPU, the existing test's bar
    return e


@pytest.mark.parametrize("api", ["host", "dev"])
@pytest.mark.parametrize("betas", dc.ADAM_BETAS, ids=str)
@pytest.mark.parametrize("step", dc.ADAM_STEPS)
def test_adam_steps_and_hyperparameters_match_float64(gpu, api, step, betas):
    worst = [0.0] * 4
    for s, b, wd, eps, gmin in dc.adam_grid():
        if (s, b) == (step, betas):
            worst = [max(a, c) for a, c in zip(worst, _grid_case(gpu, api, s, b, wd, eps, gmin))]
    print(f"adam {api} step {step} betas {betas}: p at {worst[0]:.2f} of its bar against float64 "
          f"({worst[3]:.2f} against torch), exp_avg {worst[1]:.2e}, exp_avg_sq {worst[2]:.2e} (bar 2.4e-7)")


# ---------------------------------------------------------------------------------------------------------- 4
def _special_run(gpu, api, g):
    p, _, m, v, _, _ = dc.adam_special_values()
    step, lr, b1, b2, eps, wd = dc.ADAM_SPECIAL_HYPER
    f = Flat()
    f.tensor(p, g, m, v)
    if api == "host":
        f.run(gpu, host_call(gpu, (lr, b1, b2, eps, wd), step))
    else:
        f.run(gpu, dev_call(gpu, new_state(gpu, step - 1), (lr, b1, b2, eps, wd)))
    return f.result(0)


@pytest.mark.parametrize("api", ["host", "dev"])
def test_adam_special_gradients(gpu, api):
    p, g, m, v, mask, plain_g = dc.adam_special_values()
    got = _special_run(gpu, api, g)
    want = dc.adam_torch32(p, g, m, v, *dc.ADAM_SPECIAL_HYPER)
    for a, t, name in zip(got, want, ("p", "exp_avg", "exp_avg_sq")):
        assert np.array_equal(np.isnan(a), np.isnan(t)), name           # torch's class, element for element
        assert np.array_equal(np.isposinf(a), np.isposinf(t)) and np.array_equal(np.isneginf(a), np.isneginf(t)), name
        fin = np.isfinite(t)
        if name == "p":
            assert dc.p_err(a[fin], t[fin]) <= 1.0
        else:
            assert dc.rel_err(a[fin], t[fin]) <= 2.4e-7, name
    unchanged = want[0] == p  # where torch leaves p alone (g = 0; v = inf), so does the kernel, exactly
    assert same_bits(got[0][unchanged & mask], p[unchanged & mask]) and np.any(unchanged & mask)
    assert np.any(np.isnan(want[0])) and np.any(np.isinf(want[2])) and np.any((want[0] != p) & mask & (p == 0))
    # the ordinary neighbours: the bits they get without the special values
    base = _special_run(gpu, api, plain_g)
    for a, b in zip(got, base):
        assert same_bits(a[~mask], b[~mask])
