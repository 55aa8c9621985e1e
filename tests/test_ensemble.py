"""The ensemble products on the CPU: ``mswegnn.ensemble``'s torch path against the independent
numpy restatement of tests/ensemble_cases.py (bit for bit), ``quantile_rank`` at the float
hazards, the ensemble batch builder, the chunked driver on the torch path, every wrong variant of
the restatement caught by a named case, and the C ABI's refusals (host side: they return before
any HIP call).  The reference has no counterpart for these products."""
import ctypes as C

import numpy as np
import pytest
import torch

import ensemble_cases as ec
from conftest import build_msgnn, weights
from mswegnn import _lib
from mswegnn import ensemble as ens
from mswegnn.ensemble import (EnsembleMaps, EnsembleSteps, ensemble_maps, make_ensemble, member_ranges,
                              quantile_rank, rollout_ensemble)
from mswegnn.mesh import hydrograph_bc, make_multiscale_mesh, mesh_config, wet_state
from mswegnn.metrics import finest_ranges


@pytest.fixture(scope="module")
def cases():
    return {name: ec.build_case(spec) for name, spec in ec.CASES.items()}


def ranges_of(c):
    return [(int(r), int(r) + c["n"]) for r in c["row0"]]


def np_dict(d):
    return {k: v.numpy() for k, v in d.items()}


# ------------------------------------------------------------------ the torch path == the restatement
@pytest.mark.parametrize("name", list(ec.CASES))
def test_steps_torch_equals_restatement(cases, name):
    c = cases[name]
    w = c["window"]
    want = ec.steps_reference(c["pred"], c["row0"], c["n"], c["thr"], w["t_begin"], w["t_count"])
    pred = torch.from_numpy(c["pred"])
    got = ens._steps_torch(pred[:, :, w["t_begin"]:w["t_begin"] + w["t_count"]], [int(r) for r in c["row0"]], c["n"], c["thr"])
    assert ec.same(np_dict(got), want)
    # the class: the window lands in the next columns, whatever came before
    es = EnsembleSteps(ranges_of(c), w["t_count"] + 1, c["thr"])
    es.update(pred, 0, 1).update(pred, w["t_begin"], w["t_count"])
    res = es.result()
    assert res["steps"] == w["t_count"] + 1 and res["members"] == c["M"]
    for k in ("h_mean", "h_min", "h_max"):
        assert np.array_equal(res[k][:, 1:].numpy(), want[k]), k
    for i, t in enumerate(c["thr"]):
        assert np.array_equal(res["wet_members"][t][:, 1:].numpy(), want["wet_members"][i])
        assert np.array_equal(res["wet_prob"][t].numpy(), res["wet_members"][t].numpy().astype(np.float32) / np.float32(c["M"]))


@pytest.mark.parametrize("name", list(ec.CASES))
def test_maps_torch_equals_restatement(cases, name):
    c = cases[name]
    values = torch.from_numpy(c["values"])
    for k in range(len(c["thr"])):
        steps = torch.from_numpy(c["steps"][k])
        for v, s in ((values, steps), (values, None), (None, steps)):
            want = ec.maps_reference(None if v is None else c["values"], None if s is None else c["steps"][k],
                                     c["thr"], c["ranks"])
            assert ec.same(np_dict(ens._maps_torch(v, s, c["thr"], c["ranks"])), want)


def test_restatement_is_numpys_inverted_cdf(cases):
    for name, probs in (("m3", (0.0, 0.1, 0.5, 0.9, 1.0)), ("m64", (0.0, 0.07, 0.5, 0.99, 1.0)), ("full_m7", (0.1, 0.5, 0.9))):
        c = cases[name]
        ec.check_inverted_cdf(c["values"], probs, [quantile_rank(p, c["M"]) for p in probs])


def test_ensemble_maps_public_interface(cases):
    c = cases["m64"]
    probs = (0.1, 0.5, 0.9, 0.0, 1.0)
    ranks = [quantile_rank(p, 64) for p in probs]
    assert ranks == [6, 31, 57, 0, 63]
    want = ec.maps_reference(c["values"], c["steps"][0], c["thr"], ranks)
    res = ensemble_maps(torch.from_numpy(c["values"]), torch.from_numpy(c["steps"][0]).long(), c["thr"], probs)
    assert res["members"] == 64
    for i, t in enumerate(c["thr"]):
        assert np.array_equal(res["exceed_members"][t].numpy(), want["exceed_members"][i])
        assert np.array_equal(res["exceed_prob"][t].numpy(), want["exceed_members"][i].astype(np.float32) / np.float32(64))
    assert np.array_equal(res["mean"].numpy(), want["mean"])
    assert np.array_equal(res["members_with_step"].numpy(), want["members_with_step"])
    for j, p in enumerate(probs):
        assert np.array_equal(res["quantiles"][p].numpy(), want["rank_values"][j])
        assert np.array_equal(res["step_quantiles"][p].numpy(), want["rank_steps"][j])
    with pytest.raises(ValueError):
        ensemble_maps(torch.zeros(65, 3))
    with pytest.raises(ValueError):
        ensemble_maps(torch.zeros(3, 3), probs=(0.5,) * 9)
    with pytest.raises(ValueError):
        ensemble_maps()


# ------------------------------------------------------------------ quantile_rank
@pytest.mark.parametrize("p, M, rank", [
    (0.07, 100, 6),          # 0.07 * 100 = 7.000000000000001 in float64: its ceiling would be 8
    (0.1, 10, 0), (0.3, 10, 2), (0.7, 10, 6), (0.56, 25, 13), (0.57, 100, 56), (0.29, 100, 28), (0.58, 50, 28),
    (0.5, 64, 31), (0.5, 3, 1), (0.5, 2, 0), (0.9, 10, 8), (0.1, 64, 6), (0.9, 64, 57),
    (0, 64, 0), (0.0, 1, 0), (1, 64, 63), (1.0, 1, 0), (1e-9, 64, 0), (0.999999, 64, 63),
])
def test_quantile_rank(p, M, rank):
    assert quantile_rank(p, M) == rank
    if 0 < p < 1:   # numpy's inverted_cdf on distinct values; its own float product rounds up in two of the cases
        numpy_rounds_up = (p, M) in ((0.07, 100), (0.56, 25))
        assert np.quantile(np.arange(M, dtype=np.float64), float(p), method="inverted_cdf") == rank + numpy_rounds_up


def test_quantile_rank_float_products_would_differ():
    import math
    assert math.ceil(0.07 * 100) - 1 == 7 and quantile_rank(0.07, 100) == 6
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            quantile_rank(bad, 4)
    with pytest.raises(ValueError):
        quantile_rank(0.5, 0)


# ------------------------------------------------------------------ every mutant is caught
@pytest.mark.parametrize("mutant", list(ec.STEPS_KILLED_BY))
def test_steps_mutants_are_caught(cases, mutant):
    for name in ec.STEPS_KILLED_BY[mutant]:
        c = cases[name]
        args = (c["pred"], c["row0"], c["n"], c["thr"])
        assert not ec.same(ec.step_mutants[mutant](*args, **c["window"]), ec.steps_reference(*args, **c["window"])), name


@pytest.mark.parametrize("mutant", list(ec.MAPS_KILLED_BY))
def test_maps_mutants_are_caught(cases, mutant):
    for name in ec.MAPS_KILLED_BY[mutant]:
        c = cases[name]
        args = (c["values"], c["steps"][0], c["thr"], c["ranks"])
        assert not ec.same(ec.map_mutants[mutant](*args), ec.maps_reference(*args)), name


def test_every_mutant_is_listed():
    assert set(ec.STEPS_KILLED_BY) == set(ec.STEP_MUTANTS) and set(ec.MAPS_KILLED_BY) == set(ec.MAP_MUTANTS)
    assert all(ec.STEPS_KILLED_BY.values()) and all(ec.MAPS_KILLED_BY.values())
    assert {"m3", "m64"} <= set(ec.STEPS_KILLED_BY["last_member_dropped"]) & set(ec.MAPS_KILLED_BY["last_member_dropped"])


def test_planted_cells(cases):
    c = cases["m3"]
    h, thr = c["h"], c["thr"]
    kind = np.arange(c["n"]) % ec.KINDS
    assert (h[:, kind == 0] == h[:1, kind == 0]).all() and (h[:, kind == 1] == 0).all()
    assert (c["steps"][0][:, kind == 2] == -1).all()                       # never wet at the first threshold
    assert ((h[:, kind == 3] > max(thr)).all(2).sum(0) == 1).all()         # exactly one member wet
    assert (h[:, kind == 6] > 0).all()
    assert sum((h[:, kind == 4] == np.float32(t)).any() for t in thr) == 4
    assert 0.35 < (h[:, kind >= 7] == 0).mean() < 0.55
    assert np.isnan(c["pred"][:, 1]).all() and not np.isfinite(np.delete(c["pred"][:, 0], np.concatenate(
        [np.arange(r, r + c["n"]) for r in c["row0"]]), 0)).all()
    assert list(c["row0"]) != sorted(c["row0"])


# ------------------------------------------------------------------ ensembles of graphs, the driver
@pytest.fixture(scope="module")
def tiny_model():
    return build_msgnn(num_scales=4, hid=32, K=4, state=weights("K4_F32"))


@pytest.fixture(scope="module")
def tiny_ensemble():
    g = wet_state(make_multiscale_mesh(**mesh_config("tiny"), T=9), seed=1)
    bcs = [hydrograph_bc(9, peak=p, seed=s) for p, s in ((1.0, 1), (3.0, 2), (6.0, 3))]
    return g, bcs, make_ensemble(g, bcs)


def test_make_ensemble(tiny_ensemble):
    g, bcs, b = tiny_ensemble
    ranges = member_ranges(b)
    n = finest_ranges(g)[0][1] - finest_ranges(g)[0][0]
    assert len(ranges) == 3 and {e - s for s, e in ranges} == {n} and ranges == finest_ranges(b)
    assert b.num_graphs == 3 and b.x.shape[0] == 3 * g.x.shape[0]
    for m in range(3):
        assert torch.equal(b.BC[m], torch.from_numpy(bcs[m])[0])
    xs = [g.x + m for m in range(3)]
    bx = make_ensemble(g, bcs, xs)
    assert torch.equal(bx[2].x, xs[2]) and member_ranges(bx) == ranges
    with pytest.raises(ValueError):
        make_ensemble(g, [bcs[0][:, :, :-1]])
    with pytest.raises(ValueError):
        make_ensemble(g, bcs, xs[:2])
    with pytest.raises(ValueError):
        make_ensemble(g, [bcs[0]] * 65)
    other = make_multiscale_mesh(n_coarse=3, num_scales=4, seed=5, T=9)
    from mswegnn.batch import collate
    from mswegnn.rollout import adapt_batch_training
    with pytest.raises(ValueError):
        member_ranges(adapt_batch_training(collate([g, other])))


def _same(u, v):
    if isinstance(u, dict):
        return u.keys() == v.keys() and all(_same(u[k], v[k]) for k in u)
    if not isinstance(u, torch.Tensor):
        return u == v
    if torch.is_floating_point(u):
        u, v = torch.nan_to_num(u, nan=-7.0), torch.nan_to_num(v, nan=-7.0)
    return u.dtype == v.dtype and torch.equal(u, v)


def test_rollout_ensemble_chunked_equals_whole(tiny_model, tiny_ensemble):
    _, _, b = tiny_ensemble
    probs = (0.1, 0.5, 0.9)
    whole, rw = rollout_ensemble(tiny_model, b, 9, chunk=None, probs=probs, keep_rollout=True, temporal_res=30)
    assert torch.equal(rw, tiny_model.rollout(b, 9))
    for chunk in (4, 1):
        parts, rp = rollout_ensemble(tiny_model, b, 9, chunk=chunk, probs=probs, keep_rollout=True, temporal_res=30)
        assert torch.equal(rp, rw) and _same(parts, whole), chunk
    assert whole["steps"]["steps"] == whole["maps"]["steps"] == 9 and whole["maps"]["members"] == 3
    ec.check_products(whole, rw.numpy(), member_ranges(b), (0.05, 0.3), probs, [quantile_rank(p, 3) for p in probs])
    hours = whole["maps"]["first_wet"][0.05]["arrival_hours"][0.5]
    s = whole["maps"]["first_wet"][0.05]["step_quantiles"][0.5]
    assert torch.equal(torch.isnan(hours), s < 0) and torch.equal(hours[s >= 0], s[s >= 0].double() * 30 / 60)
    # the members differ: the hydrographs reach the mesh
    assert bool((whole["steps"]["h_max"] > whole["steps"]["h_min"]).any())
    assert rollout_ensemble(tiny_model, b, 9, chunk=4, per_step=False)["steps"] is None


def test_ensemble_maps_class_reduces_other_maps(tiny_model, tiny_ensemble):
    _, _, b = tiny_ensemble
    r = tiny_model.rollout(b, 9)
    ranges = member_ranges(b)
    em = EnsembleMaps(ranges, (0.05,), (0.5,), of=("q_max", "h_max"))
    with pytest.raises(RuntimeError):
        em.result()
    res = em.update(r).result()
    n = ranges[0][1] - ranges[0][0]
    q = np.abs(np.stack([r.numpy()[s:s + n, 1, :] for s, _ in ranges])).max(2)
    assert np.array_equal(res["q_max"]["quantiles"][0.5].numpy(), ec.maps_reference(q, None, (), [1])["rank_values"][0])
    assert res["q_max"]["exceed_members"] == {} and set(res["h_max"]["exceed_members"]) == {0.05}
    with pytest.raises(ValueError):
        EnsembleMaps(ranges, of=("t_h_max",))
    with pytest.raises(ValueError):
        EnsembleSteps([(0, 4), (4, 9)], 3)


# ------------------------------------------------------------------ C ABI, host side only
@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_struct_sizes(lib):
    assert lib.msw_struct_size(b"msw_ensemble_steps_out") == C.sizeof(_lib.MswEnsembleStepsOut) == 32
    assert lib.msw_struct_size(b"msw_ensemble_maps_out") == C.sizeof(_lib.MswEnsembleMapsOut) == 40
    assert _lib.MAX_ENSEMBLE_MEMBERS == 64 and _lib.MAX_ENSEMBLE_RANKS == 8
    assert lib.msw_abi_version() == 1


def steps_call(lib, pred=1, T=8, t_begin=0, t_count=8, rows=(0, 10), M=None, n=4, thr=True, n_thr=2, T_out=8, t_out0=0,
               out=True, row0=True):
    """msw_ensemble_steps_update with dummy non-NULL addresses: every call here must return before
    anything is launched or dereferenced."""
    o = _lib.MswEnsembleStepsOut(h_mean=4096)
    th = (C.c_float * 4)(0.05, 0.3, 0, 0)
    r = (C.c_int64 * 65)(*rows)
    return lib.msw_ensemble_steps_update(C.c_void_p(4096 if pred else 0), T, t_begin, t_count, r if row0 else None,
                                         len(rows) if M is None else M, n, th if thr else None, n_thr, T_out, t_out0,
                                         C.byref(o) if out else None, None)


def maps_call(lib, M=3, n=4, thr=True, n_thr=2, ranks=(0, 2), n_ranks=None, rk=True, out=True):
    o = _lib.MswEnsembleMapsOut(mean=4096)
    th = (C.c_float * 4)(0.05, 0.3, 0, 0)
    r = (C.c_int32 * 9)(*ranks)
    return lib.msw_ensemble_maps(C.c_void_p(4096), C.c_void_p(4096), M, n, th if thr else None, n_thr,
                                 r if rk else None, len(ranks) if n_ranks is None else n_ranks,
                                 C.byref(o) if out else None, None)


STEPS_REFUSED = [
    (dict(pred=0), "null"), (dict(out=False), "null"), (dict(row0=False), "null"), (dict(thr=False), "null"),
    (dict(n_thr=5), "n_thr"), (dict(n_thr=-1), "n_thr"), (dict(M=0), "M out"), (dict(M=65), "M out"), (dict(M=-1), "M out"),
    (dict(t_begin=-1), "window"), (dict(t_begin=4, t_count=5), "window"), (dict(t_count=-1), "window"),
    (dict(T=-1, t_count=0), "window"), (dict(t_out0=-1), "columns"), (dict(t_out0=1), "columns"),
    (dict(T_out=7), "columns"), (dict(n=-1), "n negative"), (dict(rows=(0, -1)), "member_row0"),
]
MAPS_REFUSED = [
    (dict(out=False), "null"), (dict(thr=False), "null"), (dict(rk=False), "null"), (dict(n_thr=5), "n_thr"),
    (dict(n_thr=-1), "n_thr"), (dict(M=0), "M out"), (dict(M=65), "M out"), (dict(n_ranks=9), "n_ranks"),
    (dict(n_ranks=-1), "n_ranks"), (dict(ranks=(0, 3)), "rank"), (dict(ranks=(-1,)), "rank"), (dict(n=-1), "n negative"),
]


@pytest.mark.parametrize("kw, text", STEPS_REFUSED)
def test_abi_steps_rejects_bad_arguments(lib, kw, text):
    assert steps_call(lib, **kw) == -1  # MSW_ERR_INVALID
    assert text in lib.msw_last_error().decode()


@pytest.mark.parametrize("kw, text", MAPS_REFUSED)
def test_abi_maps_rejects_bad_arguments(lib, kw, text):
    assert maps_call(lib, **kw) == -1
    assert text in lib.msw_last_error().decode()


def test_abi_no_ops(lib):
    for kw in (dict(t_count=0), dict(n=0), dict(thr=False, n_thr=0, n=0), dict(t_count=0, T_out=0)):
        assert steps_call(lib, **kw) == _lib.MSW_OK
    for kw in (dict(n=0), dict(n=0, ranks=(), thr=False, n_thr=0)):
        assert maps_call(lib, **kw) == _lib.MSW_OK


@pytest.mark.parametrize("t_count", [1, 2, 4, 16, 47, 48, 100, 256, 257, 5000])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 10369, 300001, 1 << 33])
def test_abi_steps_launch_is_consistent(lib, n, t_count):
    g, r, it = ens.steps_launch(n, 16, t_count)
    assert g >= 1 and it >= 1 and 1 <= r <= 64
    assert g * r * it >= n
    assert g * r * (it - 1) < n, "iters is not minimal"
    assert g <= -(-n // r), "more workgroups than rounds"
    assert ens.steps_launch(n, 1, t_count) == (g, r, it)


def test_abi_steps_launch_edge_cases(lib):
    assert ens.steps_launch(0, 4, 8)[::2] == (0, 0) and ens.steps_launch(8, 4, 0)[::2] == (0, 0)
    g, r, it = C.c_int32(), C.c_int32(), C.c_int32()
    for n, M, t in ((-1, 4, 8), (8, 4, -1), (8, 0, 8), (8, 65, 8)):
        assert lib.msw_ensemble_steps_launch(n, M, t, C.byref(g), C.byref(r), C.byref(it)) == -1
    assert lib.msw_ensemble_steps_launch(8, 4, 8, None, C.byref(r), C.byref(it)) == -1
