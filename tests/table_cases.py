"""The "table zoo": one small model family whose categorical tables sit at every row count where a kernel changes its
path, over the QR collision counts that move the remainder table across the same switch points.  Shared by
tests/test_tables.py (the host kernels), tests/test_gpu_tables.py (the HIP forwards) and tests/test_gpu_train_tables.py
(the HIP training kernels); train_cases.CASES registers the zoo's training cases.

Row counts: 1 and 2 (every sample in one row), 63 / 64 / 65 (the sorted scatter's one-bucket-per-row form ends at 64
rows), 127 / 128 / 129 (the atomic scatter's privatised LDS sums end at 128), 200 / 201 (qr_threshold = 200: 200 stays a
plain bag, 201 is the first QR field), 255 / 256 / 257, 449, 1000 and 1031 (a prime: no c > 1 divides it).

Collision counts c: the remainder table of a QR field has c rows and its quotient table ceil(n / c), so c = 1 is one
remainder row that every sample hits, 64 / 65 either side of the one-bucket-per-row form, 129 past the privatised sums,
5000 > n one quotient row; 2, 3 and 7 leave i >= n valid (QREmbeddingBag accepts every i in [0, ceil(n / c) c))."""
import functools

import numpy as np

ROWS = [1, 2, 63, 64, 65, 127, 128, 129, 200, 201, 255, 256, 257, 449, 1000, 1031]
NUM, D, N, H = 2, 10, 64, 1
F = NUM + len(ROWS)
THRESHOLD = 200
C_ALL = (1, 2, 3, 7, 64, 65, 129, 5000)
C_FEW = (1, 7, 129)
OPS = ("mult", "add")
B_FWD, B_TRAIN = 70, 37  # 70: four 16-row tiles + 6, two 32-row tiles + 6, one 64-row tile + 6
SHAPE = dict(F=F, num=NUM, D=D, N=N, H=H, embbag=1, sizes=ROWS, threshold=THRESHOLD, edges=True)


def name(op, c, wide=False):
    """The zoo's training case in train_cases.CASES (wide: the 39-field zoo, WIDE below)."""
    return f"zoo{39 if wide else ''}_{op}_c{c}"


def train_kwargs(op, c, wide=False):
    return dict(SHAPE, **(WIDE if wide else {}), qr=1, op=op, c=c)


def valid_end(cfg, j):
    """The first invalid index of categorical field j: n for a plain table, ceil(n / c) c for a QR field."""
    n, c = cfg["feature_sizes"][cfg["numerical"] + j], cfg["qr_collisions"]
    return -(-n // c) * c if cfg["qr_flag"] and n > cfg["qr_threshold"] else n


def check_inputs(cfg, xi):
    """The helper's own claims: the three forced rows are where they should be, every index is valid, and for
    c <= 7 every remainder row of every QR field is read at least once."""
    ncat = cfg["field_size"] - cfg["numerical"]
    ends = np.array([valid_end(cfg, j) for j in range(ncat)])
    n = np.asarray(cfg["feature_sizes"][cfg["numerical"]:])
    assert not xi[0].any() and np.array_equal(xi[1], n - 1) and np.array_equal(xi[2], ends - 1)
    assert (xi >= 0).all() and (xi < ends).all()
    c = cfg["qr_collisions"]
    if cfg["qr_flag"]:
        assert (ends[n > cfg["qr_threshold"]] >= n[n > cfg["qr_threshold"]]).all()
        if c <= 7:
            for j in np.flatnonzero(n > cfg["qr_threshold"]):
                assert len(np.unique(xi[:, j] % c)) == c, (j, c)


# The 32-sample forward (fwd32_kernel) and the helper-wave training forward run only the static form: 25 K chunks
# (F D in 385 .. 400) and N = 400.  Their smallest zoo is the goldens' layout: 13 numerical fields, the 16 tables and
# ten more (tests/golden/gen_golden.py ZOO_SIZES), one hidden layer of 400.
ROWS_WIDE = ROWS + [3, 202, 203, 511, 512, 513, 777, 2047, 2048, 2499]
WIDE = dict(F=39, num=13, D=10, N=400, H=1, sizes=ROWS_WIDE)


@functools.lru_cache(maxsize=None)
def zoo(qr=1, op="mult", c=4, B=B_FWD, deep=1, seed=10, wide=False):
    """(cfg, params, xi, xv) of a zoo model for the forward tests: synth.synth_inputs with the three forced rows
    (train_cases.edge_rows).  qr = 0: the same tables as plain bags (the serving copy packs them); deep = 0: the
    MLP-free model; wide: the 39-field zoo (WIDE).  Shared between tests: read, never written."""
    import train_cases as tc
    kw = dict(SHAPE, **(WIDE if wide else {}), qr=qr, op=op, c=c, deep=deep, B=B, seed=seed)
    cfg, params, xi, xv, _ = tc.train_case(**kw)
    check_inputs(cfg, xi)
    return cfg, params, xi, xv


def first_fields(cfg):
    """(the 1-row table, a plain field, a QR field whose c does not divide n) as categorical field numbers."""
    n = cfg["feature_sizes"][cfg["numerical"]:]
    c = cfg["qr_collisions"]
    plain = next(j for j, r in enumerate(n) if 4 <= r <= cfg["qr_threshold"])  # 3 (the low bits of 2^32 + 3) valid
    qr = next(j for j, r in enumerate(n) if r > cfg["qr_threshold"] and r % c)
    return n.index(1), plain, qr


def bad_inputs(cfg, xi):
    """[(what, xi with one invalid entry)]: the first invalid index of the 1-row table, of a plain field and of a QR
    field with c not dividing n (valid_end), then -1 and 2^32 + 3 -- whose low 32 bits are a valid index, so a range
    check made after truncation misses it.  The entries sit in different rows and tiles."""
    one, plain, qr = first_fields(cfg)
    out = []
    for what, row, j, v in (("one-row table", 5, one, 1), ("plain field", 17, plain, valid_end(cfg, plain)),
                            ("qr field", 33, qr, valid_end(cfg, qr)), ("-1", 40, qr, -1),
                            ("2^32 + 3", len(xi) - 1, plain, 2 ** 32 + 3)):
        x = xi.copy()
        x[row, j] = v
        out.append((what, x))
    return out
