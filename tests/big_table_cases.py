"""Tables past 4 GiB and past 2^31 floats: the geometries, probed rows and batches of the relocation tests
(tests/test_big_table_cases.py: the claims below on the CPU, the twin against the float64 oracle, the host kernels;
tests/test_gpu_big_tables.py: every table-indexing HIP kernel).

The principle.  A *huge* model has one categorical field whose table crosses a byte or element offset at which a
32-bit product or offset wraps (2^31 B, 2^32 B, 2^31 floats, 2^33 B).  Only K <= 64 *probed rows* of that table hold
model values; every other row holds POISON.  Its *twin* is the same model with that table compacted to the K probed
rows in ascending row order, and the field's indices remapped by the monotone map row -> rank.  A kernel does the same
arithmetic on both -- only the addresses differ -- so logits, the probed rows' gradients, parameters and optimizer
state must be equal bit for bit, and everything outside the probed rows must still be POISON (parameters), or zero
(gradients, moments).  The monotone map keeps the sorted scatter's (row, sample) order and the per-row sums' order.

POISON = 1024: finite, exact in fp16, bf16 and as a row-wise int8 code (q = 127 under the scale 1024 / 127), so the
fp16 and int8 serving copies still pack; about 10^5 times a second-order weight, so a read one row off moves a logit
far past any rounding.

Geometries.
  G1     Criteo-39 shape (13 numerical + 26 categorical fields, D = 10, 3 x 400, FwFM + deep + lw); categorical field 2
         has N1 = 107,374,200 rows: emb2 4,294,968,000 B (row 53,687,091 straddles byte 2^31, row 107,374,182 byte
         2^32), emb1 0.43 GB; the serving copy's 64-B rows cross 2^31 B at row 33,554,432 and 2^32 B at row 67,108,864,
         where the 32-B fp16 rows cross 2^31 B.  Field 2 is not the last: the copy's later per-field bases and the
         trainer's later `dest` offsets lie past the crossings too.
         NOT crossed by G1: the int8 copy (16 B per row, 1.7 GB: every offset below 2^31 B) and emb1 (4 B per row; its
         byte 2^31 needs 2^29 rows).
  G1-QR  the same shape; field 2 is a QR field of 429,496,800 categories, c = 4 ("mult" / "add"): the quotient table
         has N1 rows (q * D crosses like G1), the indices stay below 2^31, and the batch reads all four remainder rows.
  G2     D = 32, one hidden layer of 400, 13 numerical + 15 categorical fields (the goldens' first 15 small tables):
         the forward sweep's D = 32 tower (test_gpu_parity) on the most fields at which the backward's LDS tile fits
         160 KiB (bwd_layout in csrc/dfwfm_train.hip: 161,792 B at F = 28, 179,344 B at F = 29; the sweep's F = 39 is
         the shape test_gpu_train.test_train_step_unsupported_shape_raises pins as refused), so G2 trains.
         Categorical field 2 has N2 = 67,108,900 rows: 8.59 GB; element offset 2^31 and byte offset 2^33 at row
         67,108,864, byte 2^32 at row 33,554,432.

What each geometry can witness.  In G1 and G1-QR only BYTE offsets wrap (the largest element offset is 1.07e9 < 2^31):
a 32-bit byte offset fails there, an `int` element product such as row * w does not.  Element products past 2^31 are
G2's, and G2 runs the kernels that take D = 32: the f32 forwards, forward_gather, the training forward and backward
(sorted and atomic scatter), plain lazy SGD and the dense optimizer step.  An `int` element product in a kernel that
runs only at D = 10 (the one-launch bf16 / int8 forwards, the serving copies) or that G2 leaves out for memory (the
touched-row lists, lazy steps with state) is witnessed by no geometry here."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np

from conftest import GOLDEN, model_kwargs

POISON = 1024.0
FIELD = 2  # the huge field, as a categorical field number (not the last)
NUM = 13
N1 = 107_374_200
N2 = 67_108_900
QR_C = 4
QR_CATEGORIES = N1 * QR_C  # 429,496,800 < 2^31
QR_THRESHOLD = 50  # the twin's field (K c categories) must stay a QR field
B_DUP = 37


def small_sizes():
    """The goldens' SMALL_SIZES (tests/golden/gen_golden.py), read from a golden's own config."""
    with np.load(os.path.join(GOLDEN, "deepfwfm_lw.npz"), allow_pickle=False) as z:
        sizes = json.loads(str(z["config"]))["feature_sizes"]
    assert len(sizes) == 39 and sizes[:NUM] == [1] * NUM
    return [int(s) for s in sizes]


def _probed(n, edges, n_random, seed):
    rows = {0, 1, n - 2, n - 1}
    for e, both in edges:
        rows |= {e - 1, e, e + 1} if both else {e - 1, e}
    r = np.random.default_rng(seed)
    while len(rows) < 4 + sum(3 if b else 2 for _, b in edges) + n_random:
        rows.add(int(r.integers(2, n - 2)))
    return np.array(sorted(rows), np.int64)


# (row, with both neighbours): the rows the module docstring names
G1_EDGES = ((53_687_091, True), (107_374_182, True), (33_554_432, False), (67_108_864, False))
G2_EDGES = ((67_108_864, True), (33_554_432, True))

GEOS = {
    "g1": SimpleNamespace(name="g1", D=10, N=400, H=3, rows=N1, edges=G1_EDGES, n_random=8, qr=None, seed=31),
    "g1qr_mult": SimpleNamespace(name="g1qr_mult", D=10, N=400, H=3, rows=N1, edges=G1_EDGES, n_random=8, qr="mult",
                                 seed=31),
    "g1qr_add": SimpleNamespace(name="g1qr_add", D=10, N=400, H=3, rows=N1, edges=G1_EDGES, n_random=8, qr="add",
                                seed=31),
    "g2": SimpleNamespace(name="g2", F=28, D=32, N=400, H=1, rows=N2, edges=G2_EDGES, n_random=4, qr=None, seed=32),
}
for _g in GEOS.values():
    _g.probed = _probed(_g.rows, _g.edges, _g.n_random, _g.seed)
    _g.K = len(_g.probed)
    _g.F = getattr(_g, "F", 39)
    _g.c = QR_C if _g.qr else 0
    _g.keys = _g.rows * QR_C if _g.qr else _g.rows  # the huge field's index range
    _g.twin_keys = _g.K * QR_C if _g.qr else _g.K


def rank_of(geo, rows):
    """The monotone map row -> rank among the probed rows (every row must be probed)."""
    rows = np.asarray(rows, np.int64)
    rank = np.searchsorted(geo.probed, rows)
    assert np.array_equal(geo.probed[rank], rows)
    return rank.astype(np.int64)


def to_twin(geo, idx):
    """The huge field's indices as the twin's: rank(row) for a plain table, rank(q) c + r for a QR field."""
    idx = np.asarray(idx, np.int64)
    if not geo.qr:
        return rank_of(geo, idx)
    return rank_of(geo, idx // QR_C) * QR_C + idx % QR_C


def cycle(geo):
    """The probed rows in the order the `dup` batch cycles through them: the rows named as edges first, so that the
    rows hit twice or more are the ones that straddle or start at a crossing."""
    first = [e for e, _ in geo.edges] + [e - 1 for e, _ in geo.edges] + [e + 1 for e, b in geo.edges if b]
    rest = [int(r) for r in geo.probed if int(r) not in first]
    out = np.array(first + rest, np.int64)
    assert len(out) == geo.K and np.array_equal(np.sort(out), geo.probed)
    return out


def huge_column(geo, kind):
    """The huge field's index column.  dup: B = 37, cycling through cycle(geo); dup_rev: the reversed cycle; once:
    B = K, every probed row exactly once in a seeded order.  QR: the remainder walks 0 .. 3 with the sample."""
    cyc = cycle(geo)
    if kind == "dup":
        rows = cyc[np.arange(B_DUP) % geo.K]
    elif kind == "dup_rev":
        rows = cyc[::-1][np.arange(B_DUP) % geo.K]
    elif kind == "once":
        rows = cyc[np.random.default_rng(geo.seed + 1).permutation(geo.K)]
    else:
        raise AssertionError(kind)
    if geo.qr:
        return rows * QR_C + (np.arange(len(rows)) * 3 + 1) % QR_C
    return rows


@functools.lru_cache(maxsize=None)
def twin(name):
    """(cfg, params) of the twin: the goldens' small tables, the huge field compacted to its K probed rows (QR: K c
    categories, a quotient table of K rows).  Shared between tests: read, never written."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    geo = GEOS[name]
    sizes = small_sizes()[:geo.F]
    sizes[NUM + FIELD] = geo.twin_keys
    cfg = dict(field_size=geo.F, feature_sizes=sizes, embedding_size=geo.D, use_fwfm=1, use_fm=0, use_logit=0,
               use_deep=1, use_lw=1, use_fwlw=0, h_depth=geo.H, deep_nodes=geo.N, numerical=NUM,
               embedding_bag=int(bool(geo.qr)), qr_flag=int(bool(geo.qr)), qr_operation=geo.qr or "mult",
               qr_collisions=QR_C, qr_threshold=QR_THRESHOLD if geo.qr else 200)
    m = DeepFMs(**model_kwargs(cfg))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    params = synth.synth_state(shapes, geo.F, geo.D, geo.N, True, True, seed=geo.seed)
    return cfg, params


def shallow(cfg, params):
    """The MLP-free FwFM model of the same tables: (cfg, params)."""
    cfg = dict(cfg, use_deep=0)
    return cfg, {k: v for k, v in params.items() if not k.startswith("net_1_")}


@functools.lru_cache(maxsize=None)
def batch(name, kind):
    """(xi_huge, xi_twin, xv, y, dlogit) of a batch: the small fields' columns from synth.synth_inputs, the huge
    field's from huge_column; y every third sample; dlogit a fixed float32 vector for the C ABI's backward."""
    from xsdeepfwfm_deprecated_amd import synth
    geo = GEOS[name]
    cfg, _ = twin(name)
    col = huge_column(geo, kind)
    B = len(col)
    xi, xv = synth.synth_inputs(cfg["feature_sizes"], NUM, B, seed=geo.seed + len(kind))
    xi_h, xi_t = xi.copy(), xi.copy()
    xi_h[:, FIELD], xi_t[:, FIELD] = col, to_twin(geo, col)
    y = (np.arange(B) % 3 == 0).astype(np.float32)
    dl = ((np.arange(B) % 7 - 3) / np.float32(8 * B)).astype(np.float32)
    dl[dl == 0] = np.float32(1.0 / (16 * B))  # every sample contributes to its rows
    return xi_h, xi_t, xv, y, dl


def table_names(geo):
    """(second-order, first-order) parameter names of the huge field's big table (QR: the quotient tables)."""
    s = "weight_q" if geo.qr else "weight"
    return f"fm_2nd_embeddings.{NUM + FIELD}.{s}", f"fm_1st_embeddings.{NUM + FIELD}.{s}"


def offsets(geo):
    """Per probed row: the byte and element offsets of its first and last byte / float in the plain table, the 64-,
    32- and 16-B copies, and first-order table; and the flat gradient layout with the huge field first (emb2, emb1,
    then every other table): (dict of [K, 2] int arrays, first float offset of the later tables)."""
    r = geo.probed
    span = lambda stride, width: np.stack([r * stride, r * stride + width - 1], axis=1)  # noqa: E731
    return dict(emb2_bytes=span(4 * geo.D, 4 * geo.D), emb2_elems=span(geo.D, geo.D), emb1_bytes=span(4, 4),
                copy64=span(64, 64), copy32=span(32, 32), copy16=span(16, 16)), geo.rows * (geo.D + 1)


def straddles(span, at):
    """Rows whose first byte / element lies below `at` and whose last lies at or past it."""
    return (span[:, 0] < at) & (span[:, 1] >= at)


def starts_at(span, at):
    return span[:, 0] == at
