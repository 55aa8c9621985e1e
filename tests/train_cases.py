"""The yardstick of the training kernels (csrc/train.hip behind mswegnn.autograd): a numpy
float64 restatement of the three functions they implement, written from the model code --

  mlp_ref     make_mlp                (models/models.py: Linear + activation after every layer)
  swegnn_ref  SWEGNN.forward          (models/gnn.py, normalize=False)
  pool_ref    MSGNN._pooling          (models/gnn.py, mean, learnable=False)

each with its hand-derived backward -- and the named cases.

Planted data.  Every input, weight and grad_out is a small integer times a power of two.  A sum
of such terms is exact in ANY order while the sum of the terms' magnitudes stays below 2^24 units
of the terms' common grid (fp32) or 2^53 (fp64): every partial sum is then an integer below the
significand's range.  ``Bound`` records, for every intermediate the kernels hold in fp32 (the
forward and d_x GEMM sums, the hop predicate's row sums, the messages and their sums, agg, ds, t,
the node pulls, the input scatter, the pooling sums) that magnitude sum over the grid unit, and
for the fp64-accumulated results (dW, db, dslope, the filter gradients) the same against 2^53;
``Bound.check`` asserts both.  The grid unit of a sum is the product of its operands' units
(``grid``: the coarsest power of two every entry is a multiple of, read off the data).  The
restatement's float64 result is then the exact real-number result, and a single cast to float32
is the only rounding -- the one the kernels perform.  Pooling: every child of a parent with c
children holds a multiple of c and grad_out[parent] is a multiple of c, so the quotients are
exact too.

The launch rules the cases aim at (csrc/train.hip, host part: gemm, weight_grad, splits_for and
split_k, blocks_for, mlp_backward) are restated below (``splits_for`` ... ``CAP``) only to place the cases
and to give the wrong variants their meaning; the correct restatement never reads them.

Each wrong ``variant`` must change a compared tensor on its named case
(tests/test_train_cases.py::test_every_wrong_variant_is_caught).
"""
import functools
import math

import numpy as np

F32_EXACT = 2.0 ** 24
F64_EXACT = 2.0 ** 53

# ------------------------------------------------------------------ launch rules (placement only)
TILE_M, TILE_N, TILE_K = 64, 64, 16
MAX_SPLITS = 256
CAP = 16384 * 256            # elements one round of an elementwise grid covers (blocks_for)


def splits_for(R):
    return min(MAX_SPLITS, max(1, R // (8 * TILE_K)))


def kchunk_for(R):
    s = splits_for(R)
    return (-(-R // s) + TILE_K - 1) // TILE_K * TILE_K


def used_splits(R):
    return max(1, -(-R // kchunk_for(R)))


def rchunk_for(R):
    return max(256, -(-R // MAX_SPLITS))


MLP_VARIANTS = ("drop_last_row", "drop_last_kslice", "last_split_unsummed", "ones_as_data", "db_rchunk_truncated",
                "drop_col64", "klanes_not_zeroed")
SWEGNN_VARIANTS = ("csr_swapped", "active_and", "upwind_gt")
POOL_VARIANTS = ("pool_cnt",)
CAP_VARIANT = "unwritten_past_cap"
VARIANTS = MLP_VARIANTS + SWEGNN_VARIANTS + POOL_VARIANTS + (CAP_VARIANT,)


# ------------------------------------------------------------------------------ exactness bound
def grid(*arrays):
    """The coarsest power of two <= 1 that every entry of every array is an integer multiple of."""
    u = 1.0
    for a in arrays:
        a = np.asarray(a, np.float64)
        if a.size == 0:
            continue
        for _ in range(80):
            v = a / u
            if np.array_equal(v, np.rint(v)):
                break
            u /= 2
        else:
            raise AssertionError("not on a dyadic grid")
    return u


class Bound:
    """Largest magnitude, in grid units, of the intermediates held in fp32 / accumulated in fp64."""

    def __init__(self):
        self.f32, self.f64 = {}, {}

    def _add(self, d, name, mag, unit):
        v = float(np.max(mag, initial=0.0)) / unit
        d[name] = max(d.get(name, 0.0), v)

    def fp32(self, name, mag, unit):
        self._add(self.f32, name, mag, unit)

    def fp64(self, name, mag, unit):
        self._add(self.f64, name, mag, unit)

    def worst(self):
        return max(self.f32.values(), default=0.0), max(self.f64.values(), default=0.0)

    def check(self):
        bad = {k: v for k, v in self.f32.items() if not v < F32_EXACT}
        bad.update({k: v for k, v in self.f64.items() if not v < F64_EXACT})
        assert not bad, f"not exact (grid units; fp32 needs < 2^24, fp64 < 2^53): {bad}"


def _mm(A, B, bound, name, plus=(), wide=False):
    """A @ B (+ the addends), recording sum |a||b| (+ |addend|) over the common grid."""
    C = A @ B
    for p in plus:
        C = C + p
    if bound is not None:
        mag = np.abs(A) @ np.abs(B)
        for p in plus:
            mag = mag + np.abs(p)
        unit = min([grid(A) * grid(B)] + [grid(p) for p in plus])
        (bound.fp64 if wide else bound.fp32)(name, mag, unit)
    return C


def _index_add(n, idx, src):
    """zeros [n, ...] with src[i] added to row idx[i]; each row's terms in index order."""
    out = np.zeros((n,) + src.shape[1:], np.float64)
    if len(idx) == 0:
        return out
    order = np.argsort(idx, kind="stable")
    si = idx[order]
    starts = np.flatnonzero(np.r_[True, si[1:] != si[:-1]])
    out[si[starts]] = np.add.reduceat(src[order], starts, axis=0)
    return out


def _flat_tail(a, start, pad):
    """a.ravel()[start + j] for j < pad, zero past the end: what a read past a row's end finds."""
    f = np.concatenate([np.asarray(a, np.float64).ravel(), np.zeros(pad + 1)])
    return f[np.minimum(start, a.size)[:, None] + np.arange(pad)[None, :]]


# ------------------------------------------------------------------------------------------ MLP
def layer(W, b=None, act=None, slope=0.25, train_W=True, train_b=True):
    """One Linear (+ activation: None, "relu", "prelu") of a make_mlp stack."""
    return dict(W=np.asarray(W, np.float64), b=None if b is None else np.asarray(b, np.float64), act=act,
                slope=float(slope), train_W=train_W, train_b=train_b)


def _mlp_forward(x, layers, variant=None, bound=None):
    h, ins, pres = np.asarray(x, np.float64), [], []
    for ly in layers:
        W, b = ly["W"], ly["b"]
        wi = W.shape[1]
        ins.append(h)
        pre = _mm(h, W.T, bound, "fwd gemm", plus=() if b is None else (b[None, :],))
        pad = (-wi) % 4
        if variant == "klanes_not_zeroed" and pad:
            xn = _flat_tail(h, np.arange(h.shape[0]) * wi + wi, pad)
            wn = _flat_tail(W, np.arange(W.shape[0]) * wi + wi, pad)
            pre = pre + xn @ wn.T
        if variant == "drop_col64":
            pre[:, 64:] = 0.0
        if variant == "drop_last_row" and len(pre):
            pre[-1] = 0.0
        pres.append(pre)
        if ly["act"] == "relu":
            h = np.where(pre > 0, pre, 0.0)
        elif ly["act"] == "prelu":
            h = np.where(pre > 0, pre, ly["slope"] * pre)
            if bound is not None:
                bound.fp32("prelu", np.abs(h), grid(h))
        else:
            assert ly["act"] is None, ly["act"]
            h = pre
    return dict(out=h, ins=ins, pres=pres)


def _rows_summed(R, variant, fused_with_dW):
    """How many leading rows a row reduction covers under a wrong variant."""
    if variant == "drop_last_row":
        return max(R - 1, 0)
    if fused_with_dW and variant == "drop_last_kslice":
        return R // kchunk_for(R) * kchunk_for(R)
    if fused_with_dW and variant == "last_split_unsummed":
        return (used_splits(R) - 1) * kchunk_for(R)
    if not fused_with_dW and variant == "db_rchunk_truncated":
        return R // rchunk_for(R) * rchunk_for(R)
    return R


def _mlp_backward(fw, layers, grad_out, need_dx=True, variant=None, bound=None):
    g = np.asarray(grad_out, np.float64)
    R = g.shape[0]
    res = {}
    for l in range(len(layers) - 1, -1, -1):
        ly, pre, xin = layers[l], fw["pres"][l], fw["ins"][l]
        W = ly["W"]
        wi = W.shape[1]
        if ly["act"] == "relu":
            dpre = np.where(pre > 0, g, 0.0)
        elif ly["act"] == "prelu":
            dpre = np.where(pre > 0, g, ly["slope"] * g)
            n = _rows_summed(R, variant, False) if variant == "drop_last_row" else R
            res[f"dslope{l}"] = np.sum(np.where(pre > 0, 0.0, pre * g)[:n]).reshape(1)
            if bound is not None:
                bound.fp32("dpre", np.abs(dpre), grid(dpre))
                bound.fp64("dslope", np.sum(np.abs(pre * g)), grid(pre) * grid(g))
        else:
            dpre = g
        if variant == "drop_last_row" and R:
            dpre = dpre.copy()
            dpre[-1] = 0.0
        fused = ly["b"] is not None and ly["train_b"] and ly["train_W"] and wi % TILE_N != 0
        if ly["train_W"]:
            n = _rows_summed(R, variant, True)
            dW = _mm(dpre[:n].T, xin[:n], bound, "dW", wide=True)
            if variant == "drop_col64":
                dW[:, 64:] = 0.0
            res[f"dW{l}"] = dW
        if ly["b"] is not None and ly["train_b"]:
            n = _rows_summed(R, variant, fused)
            if fused and variant == "ones_as_data":
                res[f"db{l}"] = dpre[:n].T @ _flat_tail(xin, np.arange(R) * wi + wi, 1)[:n, 0]
            else:
                res[f"db{l}"] = dpre[:n].sum(0)
            if bound is not None:
                bound.fp64("db", np.abs(dpre).sum(0), grid(dpre))
        if l > 0 or need_dx:
            g = _mm(dpre, W, bound, "dx gemm")
            if variant == "drop_col64":
                g[:, 64:] = 0.0
            if variant == "drop_last_row" and R:
                g[-1] = 0.0
    if need_dx:
        res["d_x"] = g
    return res


def mlp_ref(x, layers, grad_out, need_dx=True, variant=None, bound=None):
    """make_mlp over x [R, w0] and its backward for grad_out [R, wL], float64 ->
    {out, d_x, dW<l>, db<l>, dslope<l>}; d_x is absent when not wanted, dW<l> / db<l> when the
    layer's weight / bias is frozen (or there is no bias), dslope<l> unless the layer is a PReLU."""
    fw = _mlp_forward(x, layers, variant, bound)
    res = _mlp_backward(fw, layers, grad_out, need_dx, variant, bound)
    res["out"] = fw["out"]
    return res


# --------------------------------------------------------------------------------------- SWEGNN
def swegnn_ref(x_s, x_d, edge_index, edge_attr, layers, filters, K, grad_out, with_gradient=True, upwind=False,
               variant=None, bound=None):
    """SWEGNN.forward (normalize=False) and its backward, float64.  edge_index [2, E] (row = the
    sending node, col = the receiving one), edge_attr [E, ef] or None, layers: the edge MLP,
    filters: the K + 1 filter matrices or None ->
    {out, d_x_s, d_x_d, d_edge_attr, dW<l>, db<l>, dslope<l>, dfilter<k>}."""
    x_s, x_d = np.asarray(x_s, np.float64), np.asarray(x_d, np.float64)
    row, col = np.asarray(edge_index[0], np.int64), np.asarray(edge_index[1], np.int64)
    N, F = x_d.shape
    parts = [x_s[row], x_s[col], x_d[row], x_d[col]]
    if edge_attr is not None and edge_attr.shape[1] > 0:
        parts.append(np.asarray(edge_attr, np.float64))
    X0 = np.ascontiguousarray(np.concatenate(parts, 1))
    if variant == CAP_VARIANT:
        X0.reshape(-1)[CAP:] = 0.0
    mlp_variant = variant if variant in MLP_VARIANTS else None
    fw = _mlp_forward(X0, layers, mlp_variant, bound)
    s = fw["out"]
    gs = grid(s) if bound is not None else None
    out = _mm(x_d, filters[0].T, bound, "filter gemm") if filters is not None else x_d.copy()
    outs, aggs, actives, terms, passes = [], [], [], [], []
    for k in range(K):
        nz = out.sum(1) != 0                                            # the hop predicate
        active = (nz[row] & nz[col]) if variant == "active_and" else (nz[row] | nz[col])
        if with_gradient:
            d = out[col] - out[row]
            ok = (d > 0 if variant == "upwind_gt" else d >= 0) if upwind else np.ones_like(d, bool)
            term = np.where(d < 0, 0.0, d) if upwind else d
        else:
            ok = np.ones((len(row), F), bool)
            term = out[row]
        msg = np.where(active[:, None], term * s, 0.0)
        agg = _index_add(N, col, msg)
        if variant == CAP_VARIANT:
            agg.reshape(-1)[CAP:] = 0.0
        if bound is not None:
            go = grid(out)
            bound.fp32("hop predicate sum", np.abs(out).sum(1), go)
            bound.fp32("hop difference", np.abs(term), go)
            bound.fp32("agg", _index_add(N, col, np.abs(msg)), go * gs)
        outs.append(out), aggs.append(agg), actives.append(active), terms.append(term), passes.append(ok)
        out = (_mm(agg, filters[k + 1].T, bound, "filter gemm", plus=(out,)) if filters is not None else out + agg)
        if bound is not None:
            bound.fp32("out", np.abs(outs[-1]) + np.abs(out - outs[-1]), grid(out))
    res = {"out": out}
    if variant == CAP_VARIANT:
        res["out"] = out.copy()
        res["out"].reshape(-1)[CAP:] = 0.0
    G = np.asarray(grad_out, np.float64)
    ds = np.zeros((len(row), F))
    ds_mag = np.zeros((len(row), F))
    to, frm = (row, col) if variant == "csr_swapped" else (col, row)
    for k in range(K - 1, -1, -1):
        if filters is not None:
            res[f"dfilter{k + 1}"] = _mm(G.T, aggs[k], bound, "dfilter", wide=True)
            dagg = _mm(G, filters[k + 1], bound, "dagg gemm")
        else:
            dagg = G
        dm = np.where(actives[k][:, None], dagg[col], 0.0)
        ds = ds + dm * terms[k]
        t = np.where(passes[k], dm * s, 0.0)
        if with_gradient:
            Gn = G + (_index_add(N, to, t) - _index_add(N, frm, t))
        else:
            Gn = G + _index_add(N, frm, t)
        if bound is not None:
            ds_mag = ds_mag + np.abs(dm * terms[k])
            bound.fp32("ds", ds_mag, grid(dm) * grid(terms[k]))
            bound.fp32("t", np.abs(t), grid(dm) * gs)
            pulls = _index_add(N, frm, np.abs(t)) + (_index_add(N, to, np.abs(t)) if with_gradient else 0.0)
            bound.fp32("node pull", np.abs(G) + pulls, min(grid(G), grid(dm) * gs))
        G = Gn
    if filters is not None:
        res["dfilter0"] = _mm(G.T, x_d, bound, "dfilter", wide=True)
        d_xd = _mm(G, filters[0], bound, "dagg gemm")
    else:
        d_xd = G
    bw = _mlp_backward(fw, layers, ds, True, mlp_variant, bound)
    dX0 = bw.pop("d_x")
    res.update(bw)
    d_xs = _index_add(N, row, dX0[:, :F]) + _index_add(N, col, dX0[:, F:2 * F])
    d_xd = d_xd + (_index_add(N, row, dX0[:, 2 * F:3 * F]) + _index_add(N, col, dX0[:, 3 * F:4 * F]))
    if bound is not None:
        a = np.abs(dX0)
        gx = grid(dX0)
        bound.fp32("input scatter", _index_add(N, row, a[:, :F] + a[:, 2 * F:3 * F])
                   + _index_add(N, col, a[:, F:2 * F] + a[:, 3 * F:4 * F]) + np.abs(d_xd), min(gx, grid(d_xd)))
    if variant == CAP_VARIANT:
        d_xs.reshape(-1)[CAP:] = 0.0
        d_xd = d_xd.copy()
        d_xd.reshape(-1)[CAP:] = 0.0
    res["d_x_s"], res["d_x_d"] = d_xs, d_xd
    if len(parts) == 5:
        res["d_edge_attr"] = np.ascontiguousarray(dX0[:, 4 * F:])
    return res


# -------------------------------------------------------------------------------------- pooling
def pool_ref(x, pool_edges, grad_out, variant=None, bound=None):
    """Mean pooling over pool_edges [2, E] = (coarse, fine) rows and its backward ->
    {out, d_x}: out[c] = sum of x[fine] over c's edges / max(#edges of c, 1)."""
    x, g = np.asarray(x, np.float64), np.asarray(grad_out, np.float64)
    coarse, fine = np.asarray(pool_edges[0], np.int64), np.asarray(pool_edges[1], np.int64)
    N = x.shape[0]
    cnt = np.bincount(coarse, minlength=N).astype(np.float64)
    div = (cnt if variant == "pool_cnt" else np.maximum(cnt, 1.0))[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = _index_add(N, coarse, x[fine]) / div
        share = g / div
        dx = _index_add(N, fine, share[coarse])
    if bound is not None:
        bound.fp32("pool sum", _index_add(N, coarse, np.abs(x[fine])), grid(x))
        bound.fp32("pool share", _index_add(N, fine, np.abs(share[coarse])), grid(share))
        bound.fp32("pool quotient", np.abs(out), grid(out))
    if variant == CAP_VARIANT:
        out.reshape(-1)[CAP:] = 0.0
        dx.reshape(-1)[CAP:] = 0.0
    return {"out": out, "d_x": dx}


def f32(res):
    """The single rounding the kernels perform."""
    return {k: np.asarray(v).astype(np.float32) for k, v in res.items()}


# ------------------------------------------------------------------------------- planted: MLP
def _ints(rng, shape, lim, bits):
    """Integers in [-lim, lim] times 2^-bits."""
    return rng.integers(-lim, lim + 1, shape).astype(np.float64) * 2.0 ** -bits


ROWS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 385, 2049, 32767, 32768, 32769, 65535, 65537)
PAIRS = ((1, 1), (1, 32), (32, 1), (3, 5), (15, 17), (16, 16), (17, 15), (33, 50), (50, 33), (63, 64), (64, 63),
         (64, 64), (65, 2), (127, 8), (128, 8), (130, 32), (200, 50), (264, 64), (288, 64), (64, 257))


def _mlp_specs():
    c = {}
    # rows: every split-K / kchunk / rchunk / slope-partial boundary, widths <= 8; once with the
    # bias gradient fused into the weight-gradient GEMM, once with the first weight frozen (its
    # bias gradient then takes the column-sum path)
    for R in ROWS:
        c[f"rows_{R}"] = dict(R=R, widths=(6, 8, 5), acts=("prelu", None))
        c[f"rows_{R}_frozen"] = dict(R=R, widths=(6, 8, 5), acts=("prelu", "relu"), frozen=(0,))
    for wi, wo in PAIRS:
        for R in (65, 257):
            c[f"pair_{wi}_{wo}_R{R}"] = dict(R=R, widths=(wi, wo), acts=("relu",))
    for depth in (1, 2, 3):
        for bias in (True, False):
            for act in (None, "relu", "prelu"):
                c[f"depth{depth}_{'bias' if bias else 'nobias'}_{act or 'none'}"] = dict(
                    R=130, widths=(9, 12, 7, 4)[:depth + 1], acts=(act,) * depth, bias=bias)
    c["frozen_33_50"] = dict(R=257, widths=(33, 50, 3), acts=("prelu", "relu"), frozen=(0,))
    c["no_dx_17_15"] = dict(R=129, widths=(17, 15, 9), acts=("relu", "prelu"), need_dx=False)
    c["no_dx_frozen_65_2"] = dict(R=257, widths=(65, 2), acts=("prelu",), need_dx=False, frozen=(0,))
    c["slope_one_block"] = dict(R=16, widths=(5, 16), acts=("prelu",))           # R * w_out = 256
    c["slope_256_blocks"] = dict(R=32769, widths=(3, 8), acts=("prelu",))       # 4 rounds + 8 elements
    return c


MLP_SPECS = _mlp_specs()


@functools.lru_cache(maxsize=None)
def mlp_case(name, planted=True):
    """-> dict(x, layers, grad_out, need_dx): planted (dyadic) or full-precision random data."""
    sp = MLP_SPECS[name]
    rng = np.random.default_rng(abs(hash_name(name)))
    R, w, acts = sp["R"], sp["widths"], sp["acts"]
    bias, frozen = sp.get("bias", True), sp.get("frozen", ())
    layers = []
    for l in range(len(w) - 1):
        if planted:
            W = _ints(rng, (w[l + 1], w[l]), 2, 1)
            b = _ints(rng, w[l + 1], 3, 2) if bias else None
        else:
            W = rng.standard_normal((w[l + 1], w[l])) / math.sqrt(w[l])
            b = rng.standard_normal(w[l + 1]) if bias else None
        layers.append(layer(W, b, acts[l], 0.25, train_W=l not in frozen))
    if planted:
        x, g = _ints(rng, (R, w[0]), 8, 3), _ints(rng, (R, w[-1]), 3, 1)
    else:
        x, g = rng.standard_normal((R, w[0])), rng.standard_normal((R, w[-1]))
    return dict(x=x, layers=layers, grad_out=g, need_dx=sp.get("need_dx", True))


def hash_name(name):
    """A stable seed from a case name (Python's hash() is salted per process)."""
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def mlp_expected(name, planted=True, variant=None, bound=None):
    c = mlp_case(name, planted)
    return mlp_ref(c["x"], c["layers"], c["grad_out"], c["need_dx"], variant, bound)


# ---------------------------------------------------------------------------- planted: pooling
def _pool_small(F):
    return dict(N=300, F=F, parents=list(range(40, 57)), counts=list(range(17)), child_pool=(100, 300), big=False)


POOL_SPECS = {f"pool_F{F}": _pool_small(F) for F in (1, 16, 50, 64)}
# N * F = 4,198,400: the last 64 rows (elements from 4,194,304 on) are parents AND children
POOL_SPECS["pool_past_cap"] = dict(N=65600, F=64, parents=list(range(65536, 65600)),
                                   counts=[i % 16 + 1 for i in range(64)], child_pool=(64000, 65600), big=True)


@functools.lru_cache(maxsize=None)
def pool_case(name, planted=True):
    """-> dict(x, pool_edges, grad_out).  Parents with 0..16 children, rows that are neither
    parent nor child, and one fine row with two parents (of 2 and 3 children)."""
    sp = POOL_SPECS[name]
    rng = np.random.default_rng(hash_name(name))
    N, F = sp["N"], sp["F"]
    lo, hi = sp["child_pool"]
    coarse, fine = [], []
    for p, c in zip(sp["parents"], sp["counts"]):
        kids = rng.choice(np.arange(lo, hi), size=c, replace=False)
        coarse += [p] * c
        fine += [int(k) for k in kids]
    if not sp["big"]:                      # fine row 99: a child of parent 42 (2 children) and 43 (3)
        for p in (42, 43):
            fine[coarse.index(p)] = 99
    order = rng.permutation(len(coarse))
    pe = np.stack([np.asarray(coarse, np.int64)[order], np.asarray(fine, np.int64)[order]])
    cnt = np.bincount(pe[0], minlength=N)
    if planted:
        mult = np.ones(N, np.int64)        # lcm of the child counts of a row's parents
        for c, f in zip(pe[0], pe[1]):
            mult[f] = math.lcm(int(mult[f]), int(cnt[c]))
        x = _ints(rng, (N, F), 5, 2) * mult[:, None]
        g = _ints(rng, (N, F), 5, 2) * np.maximum(cnt, 1)[:, None]
    else:
        x, g = rng.standard_normal((N, F)), rng.standard_normal((N, F))
    return dict(x=x, pool_edges=pe, grad_out=g)


def pool_expected(name, planted=True, variant=None, bound=None):
    c = pool_case(name, planted)
    return pool_ref(c["x"], c["pool_edges"], c["grad_out"], variant, bound)


# ----------------------------------------------------------------------------- planted: SWEGNN
def small_graph(rng, N=203, E=640):
    """A random directed graph: rows 0..9 receive nothing (in-degree 0), rows 10..19 send nothing
    (out-degree 0), row 20 is isolated; parallel edges and self-loops may occur."""
    src = rng.integers(0, N, E)
    dst = rng.integers(0, N, E)
    src = np.where((src >= 10) & (src <= 20), src + 30, src)
    dst = np.where(dst <= 9, dst + 50, dst)
    dst = np.where(dst == 20, 77, dst)
    return np.stack([src, dst]).astype(np.int64)


def _sparse_rows(rng, shape, nnz):
    """A weight matrix with nnz entries of +-1 per row at random columns."""
    W = np.zeros(shape)
    for r in range(shape[0]):
        cols = rng.choice(shape[1], size=min(nnz, shape[1]), replace=False)
        W[r, cols] = rng.choice([-1.0, 1.0], size=len(cols))
    return W


def _swegnn_specs():
    c = {}
    i = 0
    acts = (None, "relu", "prelu")
    for F in (16, 50, 64):
        for ef in (0, 1, 16):
            for filt in (True, False):
                for grad, upwind in ((True, False), (True, True), (False, False)):
                    c[f"F{F}_ef{ef}_{'filt' if filt else 'nofilt'}_{'grad' if grad else 'nograd'}"
                      f"{'_upwind' if upwind else ''}"] = dict(
                        F=F, ef=ef, filt=filt, grad=grad, upwind=upwind, K=i % 3 + 1, depth=(i // 3) % 2 + 1,
                        act=acts[(i // 2) % 3], bias=i % 4 != 3, N=203, E=640)
                    i += 1
    c["no_edges"] = dict(F=16, ef=1, filt=True, grad=True, upwind=False, K=2, depth=2, act="prelu", bias=True,
                         N=203, E=0)
    c["no_edges_nofilt"] = dict(F=50, ef=0, filt=False, grad=False, upwind=False, K=1, depth=1, act="relu",
                                bias=True, N=203, E=0)
    # N * F = 4,198,400 with few edges, all among the last rows: the elements past the cap are checked
    c["nodes_past_cap"] = dict(F=64, ef=16, filt=True, grad=True, upwind=True, K=1, depth=1, act="prelu",
                               bias=True, N=65600, E=2000, tail=True)
    # E * F = 4,198,400 and E * w0 = 17,843,200 (five rounds) on a small node set
    c["edges_past_cap"] = dict(F=64, ef=16, filt=False, grad=True, upwind=False, K=1, depth=1, act="relu",
                               bias=True, N=4200, E=65600)
    return c


SWEGNN_SPECS = _swegnn_specs()


@functools.lru_cache(maxsize=None)
def swegnn_case(name, planted=True):
    """-> dict(x_s, x_d, edge_index, edge_attr, layers, filters, K, grad_out, with_gradient, upwind)."""
    sp = SWEGNN_SPECS[name]
    rng = np.random.default_rng(hash_name(name))
    N, E, F, ef, K = sp["N"], sp["E"], sp["F"], sp["ef"], sp["K"]
    if E == 0:
        ei = np.zeros((2, 0), np.int64)
    elif sp.get("tail"):                   # every edge among the last 200 rows (past element 4,194,304)
        ei = N - 200 + small_graph(rng, 200, E)
    elif N == 203:
        ei = small_graph(rng, N, E)
    else:
        ei = np.stack([rng.integers(0, N, E), rng.integers(0, N, E)]).astype(np.int64)
    dry = rng.random(N) < 0.3              # all-zero x_d rows: inactive and mixed edges
    w = [4 * F + ef] + [2 * F] * (sp["depth"] - 1) + [F]
    layers = []
    for l in range(sp["depth"]):
        if planted:
            W = _sparse_rows(rng, (w[l + 1], w[l]), 3 if l == 0 else 2)
            if l == 0 and ef:              # every edge_attr column feeds a fifth of the outputs
                W[:, 4 * F:] = rng.choice([-1.0, 0.0, 1.0], size=(w[1], ef), p=[0.1, 0.8, 0.1])
            b =_ints(rng, w[l + 1], 1, 0) if sp["bias"] else None
        else:
            W = rng.standard_normal((w[l + 1], w[l])) / math.sqrt(w[l])
            b = rng.standard_normal(w[l + 1]) if sp["bias"] else None
        layers.append(layer(W, b, sp["act"], 0.5))
    if planted:
        x_s, x_d = _ints(rng, (N, F), 1, 0), _ints(rng, (N, F), 1, 0)
        ea = _ints(rng, (E, ef), 1, 0) if ef else None
        filters = [_sparse_rows(rng, (F, F), 2) for _ in range(K + 1)] if sp["filt"] else None
        g = _ints(rng, (N, F), 1, 0) * (rng.random((N, F)) < 0.5)
    else:
        x_s, x_d = rng.standard_normal((N, F)), rng.standard_normal((N, F))
        ea = rng.standard_normal((E, ef)) if ef else None
        filters = [rng.standard_normal((F, F)) / math.sqrt(F) for _ in range(K + 1)] if sp["filt"] else None
        g = rng.standard_normal((N, F))
    x_d = x_d * ~dry[:, None]
    return dict(x_s=x_s, x_d=x_d, edge_index=ei, edge_attr=ea, layers=layers, filters=filters, K=K, grad_out=g,
                with_gradient=sp["grad"], upwind=sp["upwind"])


def swegnn_expected(name, planted=True, variant=None, bound=None):
    c = swegnn_case(name, planted)
    return swegnn_ref(c["x_s"], c["x_d"], c["edge_index"], c["edge_attr"], c["layers"], c["filters"], c["K"],
                      c["grad_out"], c["with_gradient"], c["upwind"], variant, bound)


# the case on which each wrong variant must show (family, case)
VARIANT_CASES = {
    "drop_last_row": [("mlp", "rows_65"), ("mlp", "rows_1_frozen")],
    "drop_last_kslice": [("mlp", "rows_2049")],              # 16 splits asked, 15 used, the last of 33 rows
    "last_split_unsummed": [("mlp", "rows_256"), ("mlp", "rows_32768")],
    "ones_as_data": [("mlp", "pair_63_64_R65"), ("mlp", "pair_127_8_R257")],
    "db_rchunk_truncated": [("mlp", "pair_64_64_R257"), ("mlp", "rows_65537_frozen"), ("mlp", "frozen_33_50")],
    "drop_col64": [("mlp", "pair_130_32_R65"), ("mlp", "pair_64_257_R65"), ("swegnn", "F64_ef16_filt_grad")],
    "klanes_not_zeroed": [("mlp", "pair_3_5_R65"), ("mlp", "pair_1_32_R65"), ("mlp", "pair_50_33_R257")],
    "csr_swapped": [("swegnn", "F16_ef0_filt_grad"), ("swegnn", "F50_ef1_nofilt_nograd")],
    "active_and": [("swegnn", "F16_ef0_filt_grad"), ("swegnn", "F64_ef16_nofilt_nograd")],
    "upwind_gt": [("swegnn", "F16_ef0_nofilt_grad_upwind"), ("swegnn", "F64_ef1_filt_grad_upwind")],
    "pool_cnt": [("pool", "pool_F1"), ("pool", "pool_F50")],
    CAP_VARIANT: [("pool", "pool_past_cap"), ("swegnn", "nodes_past_cap"), ("swegnn", "edges_past_cap")],
}

EXPECTED = {"mlp": mlp_expected, "swegnn": swegnn_expected, "pool": pool_expected}
SPECS = {"mlp": MLP_SPECS, "swegnn": SWEGNN_SPECS, "pool": POOL_SPECS}


# --------------------------------------------------- torch modules carrying a case's parameters
def _act_module(ly, dtype):
    import torch
    import torch.nn as nn
    if ly["act"] == "relu":
        return nn.ReLU()
    if ly["act"] == "prelu":
        m = nn.PReLU().to(dtype)
        with torch.no_grad():
            m.weight.fill_(ly["slope"])
        return m
    return None


def build_seq(layers, dtype):
    """The nn.Sequential make_mlp would build, holding the case's weights."""
    import torch
    import torch.nn as nn
    mods = []
    for ly in layers:
        lin = nn.Linear(ly["W"].shape[1], ly["W"].shape[0], bias=ly["b"] is not None).to(dtype)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(ly["W"]))
            if ly["b"] is not None:
                lin.bias.copy_(torch.from_numpy(ly["b"]))
        lin.weight.requires_grad_(ly["train_W"])
        mods.append(lin)
        a = _act_module(ly, dtype)
        if a is not None:
            mods.append(a)
    return nn.Sequential(*mods)


def build_swegnn(case, dtype, F, ef):
    """The drop-in's SWEGNN (models/gnn.py) holding the case's edge MLP and filters."""
    import torch
    from models.gnn import SWEGNN
    layers = case["layers"]
    lay = SWEGNN(F, F, ef, K=case["K"], normalize=False, with_filter_matrix=case["filters"] is not None,
                 with_gradient=case["with_gradient"], upwind_mode=case["upwind"], n_layers=len(layers),
                 activation=layers[0]["act"], bias=layers[0]["b"] is not None).to(dtype)
    lins = [m for m in lay.edge_mlp if isinstance(m, torch.nn.Linear)]
    slopes = [m for m in lay.edge_mlp if isinstance(m, torch.nn.PReLU)]
    assert len(lins) == len(layers)
    with torch.no_grad():
        for lin, ly in zip(lins, layers):
            assert tuple(lin.weight.shape) == ly["W"].shape, (lin.weight.shape, ly["W"].shape)
            lin.weight.copy_(torch.from_numpy(ly["W"]))
            if ly["b"] is not None:
                lin.bias.copy_(torch.from_numpy(ly["b"]))
        for m, ly in zip(slopes, layers):
            m.weight.fill_(ly["slope"])
        if case["filters"] is not None:
            for f, W in zip(lay.filter_matrix, case["filters"]):
                f.weight.copy_(torch.from_numpy(W))
    return lay


def module_grads(res_keys, layers, lins, slopes, filters=None):
    """Gradients of torch modules under the restatement's names."""
    out = {}
    for l, lin in enumerate(lins):
        if f"dW{l}" in res_keys:
            out[f"dW{l}"] = lin.weight.grad
        if f"db{l}" in res_keys:
            out[f"db{l}"] = lin.bias.grad
    it = iter(slopes)
    for l, ly in enumerate(layers):
        if ly["act"] == "prelu":
            out[f"dslope{l}"] = next(it).weight.grad
    for k, f in enumerate(filters or ()):
        out[f"dfilter{k}"] = f.weight.grad
    return out
