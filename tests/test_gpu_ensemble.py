"""The ensemble kernels (msw_ensemble_steps_update, msw_ensemble_maps) on the GPU against the numpy
restatement of tests/ensemble_cases.py -- the reference has no counterpart for these products.
Every output is exact (counts, selected values, minima, maxima) or a float32 rounding of an fp64
sum added in member order, so everything is compared with ``torch.equal``, also however the
horizon is cut into windows.  Every output array sits between canary words, and columns outside a
call's window must keep theirs.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ensemble_cases as ec
from conftest import build_msgnn, weights
from mswegnn import _lib
from mswegnn.ensemble import (EnsembleMaps, EnsembleSteps, ensemble_maps, make_ensemble, member_ranges, quantile_rank,
                              rollout_ensemble, steps_launch)
from mswegnn.mesh import hydrograph_bc, make_multiscale_mesh, mesh_config

pytestmark = pytest.mark.gpu

PAD = 37          # canary words on each side of every output array: the arrays are not 16-byte aligned
PAD_ALIGNED = 40  # ... or are, and a leading stride and first column that are multiples of 4 allow 16-byte stores
NS, MS = (1, 63, 64, 65, 257), (1, 2, 3, 63, 64)


class Buffers:
    """The output arrays ``{name: shape}`` (int32 for the names of ``ints``), each inside a
    canary-filled allocation."""

    def __init__(self, shapes, ints, dev, pad=PAD):
        self.full, self.view, self.pad = {}, {}, pad
        for k, shape in shapes.items():
            size = int(np.prod(shape))
            if k in ints:
                self.full[k] = torch.full((size + 2 * pad,), int(ec.CANARY_I), device=dev, dtype=torch.int32)
            else:
                self.full[k] = torch.full((size + 2 * pad,), float(ec.CANARY_F), device=dev, dtype=torch.float32)
            self.view[k] = self.full[k][pad:pad + size].view(shape)

    def pointers(self):
        return {k: v.data_ptr() for k, v in self.view.items() if v.numel()}

    def check(self, want, label=""):
        """The pads hold their canaries and every array equals ``want`` (which holds the canary in
        the columns that the call must not touch)."""
        for k, b in self.full.items():
            c = float(ec.CANARY_F) if b.is_floating_point() else int(ec.CANARY_I)
            assert bool((b[:self.pad] == c).all()) and bool((b[-self.pad:] == c).all()), f"{label}: {k}: canary overwritten"
            w = torch.from_numpy(np.ascontiguousarray(want[k]))
            got = self.view[k].cpu()
            assert got.dtype == w.dtype and got.shape == w.shape and torch.equal(got, w), f"{label}: {k}"

    def untouched(self):
        return all(bool((b == (float(ec.CANARY_F) if b.is_floating_point() else int(ec.CANARY_I))).all())
                   for b in self.full.values())


def steps_buffers(n, n_thr, T_out, dev, want=ec.STEP_NAMES, pad=PAD):
    shapes = {k: (n_thr, n, T_out) if k == "wet_members" else (n, T_out) for k in want}
    return Buffers(shapes, ("wet_members",), dev, pad)


def steps_update(pred, row0, n, thr, bufs, t_begin, t_count, T_out, t_out0, stream=None, M=None, n_thr=None, T=None):
    th = (C.c_float * 8)(*thr)
    o = _lib.MswEnsembleStepsOut(**bufs.pointers())
    r = (C.c_int64 * 65)(*[int(v) for v in row0])
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    return _lib.lib().msw_ensemble_steps_update(C.c_void_p(pred.data_ptr()), pred.shape[2] if T is None else T, t_begin,
                                                t_count, r,
                                                len(row0) if M is None else M, n, th,
                                                len(thr) if n_thr is None else n_thr, T_out, t_out0, C.byref(o), st)


def run_steps(host, dev, row0, n, thr, t_begin=0, t_count=None, T_out=None, t_out0=0, want=ec.STEP_NAMES, pad=PAD,
              label=""):
    """One raw ABI call into canary buffers, checked against the restatement."""
    t_count = host.shape[2] - t_begin if t_count is None else t_count
    T_out = t_count if T_out is None else T_out
    bufs = steps_buffers(n, len(thr), T_out, dev.device, want, pad)
    _lib.check(steps_update(dev, row0, n, thr, bufs, t_begin, t_count, T_out, t_out0))
    ref = ec.steps_reference(host, row0, n, thr, t_begin, t_count, T_out, t_out0)
    bufs.check({k: ref[k] for k in want}, label)


def on_device(host, cuda, shift=0):
    """``host`` [N, 2, T] on the GPU, its base ``shift`` floats past a 16-byte boundary."""
    store = torch.zeros(host.size + 8, device=cuda)
    dev = store[shift:shift + host.size].view(host.shape)
    dev.copy_(torch.from_numpy(host))
    assert dev.data_ptr() % 16 == (4 * shift) % 16
    return dev


# ------------------------------------------------------------------ 1. kernel A: shape sweep
@pytest.mark.parametrize("T", [1, 47, 48, 65, 130])
def test_steps_shape_sweep(cuda, T):
    """T = 48 takes the 16-byte loader from an aligned base, every other T and every shifted base
    the scalar one; outputs whose leading stride and first column are multiples of 4 take 16-byte
    stores (canary pads of 40 words; 37 elsewhere).  Every (n, M) runs the whole window with all
    outputs and four thresholds, and one of five further variants."""
    for i_n, n in enumerate(NS):
        for i_m, M in enumerate(MS):
            label = f"n={n} M={M} T={T}"
            host, row0 = ec.place(ec.make_members(n, M, T, seed=T + n + M), seed=n + M)
            dev = on_device(host, cuda)
            run_steps(host, dev, row0, n, ec.THR4, pad=PAD_ALIGNED, label=label)
            variant = (i_n + i_m) % 5
            if variant == 0:    # a base that is not 16-byte aligned, columns t_out0 > 0 of a wider output
                run_steps(host, on_device(host, cuda, 1), row0, n, ec.THR4[:2], 0, T, T + 9, 5, label=label + " shifted")
            elif variant == 1:  # a window that starts at an odd step, of odd length, no thresholds
                tb = min(3, T - 1)
                tc = max((T - tb) // 2 * 2 - 1, 1)
                run_steps(host, dev, row0, n, (), tb, tc, tc + 4, 3, label=label + f" window=({tb}, {tc})")
            elif variant == 2:  # a window from a multiple of 4 into aligned columns: 16-byte loads and stores
                tb = min(4, T - 1)
                tc = T - tb - (T > 8)
                run_steps(host, dev, row0, n, ec.THR4[:2], tb, tc, (tc + 11) // 4 * 4, 4, pad=PAD_ALIGNED,
                          label=label + f" window=({tb}, {tc})")
            elif variant == 3:  # each output alone
                for k in ec.STEP_NAMES:
                    run_steps(host, dev, row0, n, ec.THR4[:2], want=(k,), label=label + " " + k)
            else:               # the horizon in windows of 1, 16 and 17 steps equals the whole
                whole = ec.steps_reference(host, row0, n, ec.THR4[:2])
                for step in (1, 16, 17):
                    bufs = steps_buffers(n, 2, T, cuda)
                    for t0 in range(0, T, step):
                        _lib.check(steps_update(dev, row0, n, ec.THR4[:2], bufs, t0, min(step, T - t0), T, t0))
                    bufs.check(whole, label + f" windows of {step}")


@pytest.mark.parametrize("name", list(ec.CASES))
def test_steps_named_cases(cuda, name):
    c = ec.build_case(ec.CASES[name])
    run_steps(c["pred"], on_device(c["pred"], cuda), c["row0"], c["n"], c["thr"], label=name, **c["window"])


def test_steps_repeat_and_duplicate_member(cuda):
    """A range may repeat (that member counts twice), and two calls give the same bits."""
    host, row0 = ec.place(ec.make_members(65, 3, 48, seed=7), seed=7)
    row0 = np.array([row0[2], row0[0], row0[2], row0[1]])
    dev = on_device(host, cuda)
    for _ in range(2):
        run_steps(host, dev, row0, 65, ec.THR4)


# ------------------------------------------------------------------ 2. kernel A: the cell loop
@pytest.mark.parametrize("rounds", [2, 3])
def test_steps_several_rounds_per_workgroup(cuda, rounds):
    M, T = 2, 2
    n = ec.cells_for_rounds(steps_launch, M, T, rounds)
    grid, per_wg, iters = steps_launch(n, M, T)
    assert iters == rounds and grid * per_wg * (iters - 1) < n < grid * per_wg * iters
    host, row0 = ec.place(ec.make_members(n, M, T, seed=rounds), seed=rounds)
    assert host.nbytes < 32 << 20
    run_steps(host, on_device(host, cuda), row0, n, ec.THR4[:2], label=f"n={n} grid={grid} iters={iters}")


# ------------------------------------------------------------------ 3. kernel B
def maps_call(values, steps, M, n, thr, ranks, bufs, n_ranks=None, n_thr=None):
    th = (C.c_float * 8)(*thr)
    o = _lib.MswEnsembleMapsOut(**bufs.pointers())
    rk = (C.c_int32 * 9)(*ranks)
    return _lib.lib().msw_ensemble_maps(C.c_void_p(values.data_ptr() if values is not None else 0),
                                        C.c_void_p(steps.data_ptr() if steps is not None else 0), M, n, th,
                                        len(thr) if n_thr is None else n_thr, rk,
                                        len(ranks) if n_ranks is None else n_ranks, C.byref(o),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))


def maps_buffers(n, n_thr, n_ranks, dev, names=ec.MAP_NAMES):
    shapes = {"exceed_members": (n_thr, n), "mean": (n,), "rank_values": (n_ranks, n), "members_with_step": (n,),
              "rank_steps": (n_ranks, n)}
    return Buffers({k: shapes[k] for k in names}, ("exceed_members", "members_with_step", "rank_steps"), dev)


def run_maps(values, steps, thr, ranks, cuda, label=""):
    src = values if values is not None else steps
    M, n = src.shape
    names = [k for k in ec.MAP_NAMES if (values is not None and k in ec.MAP_NAMES[:3]) or (steps is not None and k in ec.MAP_NAMES[3:])]
    bufs = maps_buffers(n, len(thr), len(ranks), cuda, names)
    dv = None if values is None else torch.from_numpy(values).to(cuda)
    ds = None if steps is None else torch.from_numpy(steps).to(cuda)
    _lib.check(maps_call(dv, ds, M, n, thr, ranks, bufs))
    bufs.check(ec.maps_reference(values, steps, thr, ranks), label)


@pytest.mark.parametrize("M", MS)
def test_maps_shape_sweep(cuda, M):
    for n in NS:
        values, steps = ec.member_maps(ec.make_members(n, M, 5, seed=M + n), ec.THR4)
        rank_sets = ((0,), (M - 1,), (0, 0), tuple(int(r) for r in np.linspace(0, M - 1, 8).round()))
        for j, ranks in enumerate(rank_sets):
            label = f"n={n} M={M} ranks={ranks}"
            run_maps(values, steps[j], ec.THR4[:(0, 2, 4, 4)[j]], ranks, cuda, label)
            run_maps(values, None, ec.THR4[:2], ranks, cuda, label + " values only")
            run_maps(None, steps[j], (), ranks, cuda, label + " steps only")
        run_maps(values, steps[0], ec.THR4, (), cuda, f"n={n} M={M} no ranks")


@pytest.mark.parametrize("name", list(ec.CASES))
def test_maps_named_cases(cuda, name):
    c = ec.build_case(ec.CASES[name])
    for k in range(len(c["thr"])):
        run_maps(c["values"], c["steps"][k], c["thr"], c["ranks"], cuda, f"{name} thr {k}")


def test_maps_several_rounds_per_workgroup(cuda):
    n = 64 * 4096 * 2 + 64 * 1000 + 13     # two full rounds of the capped grid and a ragged third
    values, steps = ec.member_maps(ec.make_members(n, 2, 2, seed=3), ec.THR4[:1])
    run_maps(values, steps[0], ec.THR4[:1], (0, 1), cuda, f"n={n}")


def test_ensemble_maps_public_interface(cuda):
    values, steps = ec.member_maps(ec.make_members(257, 7, 5, seed=11), ec.THR4[:2])
    probs = (0.1, 0.5, 0.9)
    ranks = [quantile_rank(p, 7) for p in probs]
    res = ensemble_maps(torch.from_numpy(values).to(cuda), torch.from_numpy(steps[1]).to(cuda), ec.THR4[:2], probs)
    want = ec.maps_reference(values, steps[1], ec.THR4[:2], ranks)
    for j, p in enumerate(probs):
        assert torch.equal(res["quantiles"][p].cpu(), torch.from_numpy(want["rank_values"][j]))
        assert torch.equal(res["step_quantiles"][p].cpu(), torch.from_numpy(want["rank_steps"][j]))
    assert torch.equal(res["mean"].cpu(), torch.from_numpy(want["mean"]))
    assert torch.equal(res["exceed_members"][0.25].cpu(), torch.from_numpy(want["exceed_members"][1]))
    assert torch.equal(res["members_with_step"].cpu(), torch.from_numpy(want["members_with_step"]))


# ------------------------------------------------------------------ 4. refusals leave the outputs alone
def test_abi_refusals_keep_the_canaries(cuda):
    lib = _lib.lib()
    n, M, T = 5, 3, 8
    host, row0 = ec.place(ec.make_members(n, M, T, seed=1), seed=1)
    dev = on_device(host, cuda)
    bufs = steps_buffers(n, 2, T, cuda)
    thr = ec.THR4[:2]
    ok = dict(pred=dev, row0=row0, n=n, thr=thr, bufs=bufs, t_begin=0, t_count=T, T_out=T, t_out0=0)
    bad = [dict(M=65), dict(M=0), dict(t_begin=-1), dict(t_begin=4, t_count=5), dict(t_count=-1), dict(t_out0=-1),
           dict(t_out0=1), dict(T_out=7), dict(n=-1), dict(row0=np.array([0, -1, 3])), dict(thr=ec.THR4 + (2.0,)), dict(n_thr=-1), dict(T=-1)]
    for kw in bad:
        assert steps_update(**{**ok, **kw}) == -1, kw      # MSW_ERR_INVALID
        assert bufs.untouched(), kw
    th, r = (C.c_float * 4)(*ec.THR4), (C.c_int64 * 3)(*[int(v) for v in row0])
    o, st = _lib.MswEnsembleStepsOut(**bufs.pointers()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = C.c_void_p(dev.data_ptr())
    for args in ((None, T, 0, T, r, M, n, th, 2, T, 0, C.byref(o), st), (p, T, 0, T, None, M, n, th, 2, T, 0, C.byref(o), st),
                 (p, T, 0, T, r, M, n, None, 2, T, 0, C.byref(o), st), (p, T, 0, T, r, M, n, th, 2, T, 0, None, st)):
        assert lib.msw_ensemble_steps_update(*args) == -1 and "null" in lib.msw_last_error().decode()
    assert bufs.untouched()
    for kw in (dict(t_count=0), dict(n=0)):                # no-ops
        assert steps_update(**{**ok, **kw}) == _lib.MSW_OK and bufs.untouched()
    _lib.check(steps_update(**ok))                         # and the good call still works
    bufs.check(ec.steps_reference(host, row0, n, thr))

    values, steps = ec.member_maps(ec.make_members(n, M, T, seed=1), thr)
    dv, ds = torch.from_numpy(values).to(cuda), torch.from_numpy(steps[0]).to(cuda)
    mb = maps_buffers(n, 2, 2, cuda)
    okm = dict(values=dv, steps=ds, M=M, n=n, thr=thr, ranks=(0, 2), bufs=mb)
    for kw in (dict(ranks=(0, M)), dict(ranks=(-1, 0)), dict(M=65), dict(M=0), dict(n=-1), dict(n_ranks=9), dict(n_ranks=-1),
               dict(thr=ec.THR4 + (2.0,)), dict(n_thr=-1)):
        assert maps_call(**{**okm, **kw}) == -1, kw
        assert mb.untouched(), kw
    assert maps_call(**{**okm, "n": 0}) == _lib.MSW_OK and mb.untouched()
    _lib.check(maps_call(**okm))
    mb.check(ec.maps_reference(values, steps[0], thr, (0, 2)))


# ------------------------------------------------------------------ 5. the engine, end to end
@pytest.fixture(scope="module")
def engine(cuda):
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    m.engine = "hip"
    return m


@pytest.fixture(scope="module")
def ensemble(cuda):
    g = make_multiscale_mesh(**mesh_config("small"), T=48)
    bcs = [hydrograph_bc(48, peak=p, seed=s) for p, s in ((1.0, 1), (3.0, 2), (4.5, 3), (7.0, 4))]
    return make_ensemble(g, bcs).to(cuda)


def _same(u, v):
    if isinstance(u, dict):
        return u.keys() == v.keys() and all(_same(u[k], v[k]) for k in u)
    if not isinstance(u, torch.Tensor):
        return u == v
    return u.dtype == v.dtype and torch.equal(u, v)


def test_rollout_ensemble(cuda, engine, ensemble):
    probs = (0.1, 0.5, 0.9)
    chunked, rc = rollout_ensemble(engine, ensemble, 48, chunk=16, probs=probs, keep_rollout=True)
    whole, rw = rollout_ensemble(engine, ensemble, 48, chunk=None, probs=probs, keep_rollout=True)
    assert torch.equal(rc, rw) and _same(chunked, whole)
    ranges = member_ranges(ensemble)
    assert len(ranges) == 4
    ec.check_products(whole, rw.cpu().numpy(), ranges, (0.05, 0.3), probs, [quantile_rank(p, 4) for p in probs],
                      to_np=lambda t: t.cpu().numpy())
    assert bool((whole["steps"]["h_max"] > whole["steps"]["h_min"]).any())   # the hydrographs reach the mesh


def test_update_behind_rollout_on_a_side_stream(cuda, engine, ensemble):
    from mswegnn.engine import plan_for
    probs = (0.5,)
    want, whole = rollout_ensemble(engine, ensemble, 48, chunk=None, probs=probs, keep_rollout=True)
    ranges = member_ranges(ensemble)
    plan = plan_for(engine, ensemble)
    side = torch.cuda.Stream(cuda)
    es = EnsembleSteps(ranges, 48, device=cuda)
    em = EnsembleMaps(ranges, probs=probs, of=("h_max", "first_wet"), device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = plan.rollout(ensemble.x, ensemble.BC, ensemble.node_BC, ensemble.type_BC, 48)
        es.update(out)       # enqueued directly behind the rollout: no synchronisation in between
        em.update(out)
        maps = em.result()
    side.synchronize()
    assert torch.equal(out, whole)
    assert _same(es.result(), want["steps"]) and _same(maps, want["maps"])
