"""The flood-map kernel (msw_flood_maps_update) on the GPU, compared EXACTLY (torch.equal):
against the reference's functions (tests/golden/fx_floodmaps.npz) and against the torch
restatement ``_maps_torch`` evaluated on the CPU.  Counts, steps, maxima and their steps are
exact by construction; vel_max too, because fp32 division is correctly rounded under the build's
flags (no fast-math) and nothing in q / h, 9.81f * h, vel / sqrtf(.) can contract into an FMA.

froude_max is the one map where the CPU yardstick itself is not exact.  Measured on the MI355X:
every array of the first fixture rollout equal except froude_max, 8 of 1,534 rows off by at
most 2 ulp.  The operation is the square root, and the side is the CPU's: ``torch.sqrt`` on a
CPU float32 tensor (the build's vectorised math library) is faithfully, not correctly, rounded
-- on that rollout 323 (cell, step) values are 1 ulp from sqrt evaluated in float64 and rounded
once, which numpy's float32 sqrt and the kernel's sqrtf (v_sqrt_f32 plus the +-1 ulp fix-up
sequence in its ISA) both reproduce; product and divisions agree bit for bit.  So froude_max is
checked twice:
  * EXACTLY against ``ieee_froude_max``: the same expression with that one sqrt correctly
    rounded (float64 sqrt of the float32 product, rounded once: 53 >= 2 * 24 + 2 bits);
  * within FROUDE_ULP = 3 of the reference fixture / ``_maps_torch``.  The bound comes from the
    reference's own error: its sqrt s' = s (1 + d), |d| <= 2^-23 (1 ulp), moves the quotient
    x = vel / s by at most 2^-23 x <= 2 ulp(x) (ulp(x) >= 2^-24 x), and rounding x and x' to
    nearest adds at most half an ulp each; a maximum over time moves no further than its terms.
Then: the engine's rollout run in chunks against the whole rollout, bit for bit, and reduced to
maps chunk by chunk.

The staging geometry (rows per round x time parts, tests/floodmaps_cases.py) changes at 33, 66, 132,
264 and 528 steps, and each class runs with the 16-byte and the scalar loader:
``test_every_geometry_equals_maps_torch`` steps over every edge with both, with rows planted at
the part and slab boundaries of the launch that reduces them, and ``test_carry_over_across_parts_and_slabs``
cuts the long classes inside a part, on a part boundary and at the 1024-step slab.
"""
import ctypes as C

import pytest
import torch

import floodmaps_cases as fc
from conftest import build_msgnn, golden, weights
from floodmaps_cases import EPS, THR4, f32, make_rollout
from mswegnn import _lib
from mswegnn.batch import collate
from mswegnn.floodmaps import MAP_NAMES, FloodMaps, _maps_torch, flood_maps, rollout_chunks, rollout_flood_maps
from mswegnn.mesh import make_multiscale_mesh, mesh_config, wet_state
from mswegnn.metrics import finest_ranges
from mswegnn.rollout import adapt_batch_training

pytestmark = pytest.mark.gpu

FX = golden("fx_floodmaps")
PAD = 37          # canary words on each side of every output array
CANARY_F, CANARY_I = -12345.5, -123456789
POISON = 7.0e8    # rows outside the requested range: reading one would change a maximum


FROUDE_ULP = 3


def ieee_froude_max(pred, eps=EPS):
    """froude_max of pred [n, 2, T] (CPU) with every operation correctly rounded."""
    h, q = pred[:, 0, :], pred[:, 1, :].abs()
    vel = q / h
    vel[h <= eps] = 0
    fr = vel / torch.sqrt((9.81 * h).double()).float()
    fr[h <= 0] = 0
    return fr.max(1).values


def ulps(a, b):
    """Largest distance in units in the last place between two non-negative float32 tensors."""
    return int((a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs().max())


def expected(rows, thr, t_offset=0):
    """The yardsticks for rollout rows [n, 2, T] on the CPU: _maps_torch plus the IEEE Froude map."""
    want = _maps_torch(rows, thr, EPS, t_offset)
    want["froude_ieee"] = ieee_froude_max(rows)
    return want


def check_map(k, got, want, label=""):
    got = got.cpu()
    if k == "froude_max":
        assert torch.equal(got, want["froude_ieee"]), f"{label}: froude_max vs correctly rounded arithmetic"
        d = ulps(got, want[k])
        assert d <= FROUDE_ULP, f"{label}: froude_max {d} ulp from the torch composition"
    else:
        assert torch.equal(got, want[k]), f"{label}: {k}"


class Buffers:
    """Every output array inside a canary-filled allocation."""

    def __init__(self, nrows, n_thr, dev, want=MAP_NAMES):
        self.full, self.view = {}, {}
        for k in want:
            thr_map = k in ("wet_steps", "first_wet", "last_wet")
            if thr_map and n_thr == 0:
                continue
            flt = k in ("h_max", "q_max", "vel_max", "froude_max")
            size = nrows * (n_thr if thr_map else 1)
            self.full[k] = torch.full((size + 2 * PAD,), CANARY_F if flt else CANARY_I, device=dev,
                                      dtype=torch.float32 if flt else torch.int32)
            v = self.full[k][PAD:PAD + size]
            self.view[k] = v.view(n_thr, nrows) if thr_map else v

    def struct(self):
        return _lib.MswFloodMaps(**{k: v.data_ptr() for k, v in self.view.items()})

    def check_canaries(self):
        for k, b in self.full.items():
            c = CANARY_F if b.is_floating_point() else CANARY_I
            assert bool((b[:PAD] == c).all()) and bool((b[-PAD:] == c).all()), f"{k}: canary overwritten"


def update(pred, bufs, t_begin, t_count, t_offset, row0, nrows, thr, first=1, stream=None):
    th = (C.c_float * 4)(*(list(thr) + [0.0] * (4 - len(thr))))
    m = bufs.struct()
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().msw_flood_maps_update(C.c_void_p(pred.data_ptr()), pred.shape[2], t_begin, t_count,
                                                t_offset, row0, nrows, th, len(thr), EPS, first, C.byref(m), st))


def assert_maps(bufs, want, n_thr, label):
    bufs.check_canaries()
    for k, v in bufs.view.items():
        check_map(k, v, want, label)
    if n_thr == 0:
        assert not set(bufs.view) & {"wet_steps", "first_wet", "last_wet"}


@pytest.mark.parametrize("name", [str(n) for n in FX["rollouts"]])
def test_kernel_equals_reference_fixture(cuda, name):
    r = torch.from_numpy(golden(name)["rollout"]).to(cuda)
    thr = (0.0, 0.05, 0.3)
    tres = torch.from_numpy(FX["temporal_res"])
    res = flood_maps(r, thresholds=thr, temporal_res=tres, time_start=2)
    want = {k: torch.from_numpy(FX[f"{name}/{k}"]) for k in ("h_max", "t_h_max", "q_max", "t_q_max", "vel_max",
                                                            "froude_max")}
    want["froude_ieee"] = ieee_froude_max(r.cpu())
    for k in ("h_max", "t_h_max", "q_max", "t_q_max", "vel_max", "froude_max"):
        check_map(k, res[k], want, name)
    for t in thr:
        for k in ("wet_steps", "first_wet", "last_wet"):
            assert torch.equal(res[k][t].cpu(), torch.from_numpy(FX[f"{name}/{k}_{t}"])), (k, t)
        assert torch.equal(res["fat_hours"][t].cpu(), torch.from_numpy(FX[f"{name}/fat_{t}_2"])), t


# (T, t_begin, t_count): whole windows (even T from an aligned base: 16-byte loads; odd T: the
# scalar loader), a partial window, and a window longer than one launch takes (1024 steps)
WINDOWS = [(1, 0, 1), (3, 0, 3), (7, 0, 7), (8, 0, 8), (48, 0, 48), (50, 0, 50), (50, 3, 44), (1100, 0, 1100)]


@pytest.mark.parametrize("T, t_begin, t_count", WINDOWS)
def test_shape_sweep_equals_maps_torch(cuda, T, t_begin, t_count):
    sizes = (1, 63, 64, 65, 257, 1499) if T <= 50 else (1, 65)
    total = max(sizes) + 5 + 3
    host = make_rollout(total, T, seed=T)
    for nrows in sizes:
        for row0 in (0, 5):
            inside = host.clone()
            inside[:row0] = POISON
            inside[row0 + nrows:] = POISON
            dev = inside.to(cuda)
            for n_thr in (0, 1, 4):
                thr = THR4[:n_thr]
                want = expected(host[row0:row0 + nrows, :, t_begin:t_begin + t_count], thr, 11)
                bufs = Buffers(nrows, n_thr, cuda)
                update(dev, bufs, t_begin, t_count, 11, row0, nrows, thr)
                assert_maps(bufs, want, n_thr, f"nrows={nrows} row0={row0} n_thr={n_thr}")


@pytest.mark.parametrize("case", fc.CASES, ids=[c.id for c in fc.CASES])
def test_every_geometry_equals_maps_torch(cuda, case):
    sizes = case.row_counts()
    total = max(sizes) + 5 + 3
    T, tb, tc = case.T, case.t_begin, case.t_count
    host = fc.case_rollout(case, total)
    whole = expected(host[:, :, tb:tb + tc], THR4, fc.T_OFFSET)     # rows reduce independently: computed once
    store = torch.zeros(total * 2 * T + 8, device=cuda)
    dev = store[case.shift:case.shift + total * 2 * T].view(total, 2, T)
    assert dev.data_ptr() % 16 == (4 * case.shift) % 16
    for nrows in sizes:
        for row0 in (0, 5):
            inside = host.clone()
            inside[:row0] = POISON
            inside[row0 + nrows:] = POISON
            dev.copy_(inside)
            want = {k: v[..., row0:row0 + nrows] for k, v in whole.items()}
            for n_thr in (0, 4):
                bufs = Buffers(nrows, n_thr, cuda)
                update(dev, bufs, tb, tc, fc.T_OFFSET, row0, nrows, THR4[:n_thr])
                assert_maps(bufs, want, n_thr, f"{case.id} nrows={nrows} row0={row0} n_thr={n_thr}")


def test_misaligned_base_takes_the_scalar_loader(cuda):
    T, n = 48, 257
    host = make_rollout(n, T, seed=3)
    store = torch.zeros(n * 2 * T + 8, device=cuda)
    for shift in (1, 2, 4):  # 4 floats = 16 bytes: aligned again
        dev = store[shift:shift + n * 2 * T].view(n, 2, T)
        dev.copy_(host)
        assert dev.data_ptr() % 16 == (4 * shift) % 16
        bufs = Buffers(n, 2, cuda)
        update(dev, bufs, 0, T, 0, 0, n, THR4[:2])
        assert_maps(bufs, expected(host, THR4[:2]), 2, f"shift={shift}")


def test_several_row_loop_iterations(cuda):
    T = 4
    g, r, it = C.c_int32(), C.c_int32(), C.c_int32()
    lib = _lib.lib()
    _lib.check(lib.msw_flood_maps_launch(1 << 40, T, C.byref(g), C.byref(r), C.byref(it)))
    nrows = g.value * r.value * 2 + r.value * (g.value // 3) + 13   # two full rounds and a ragged third
    _lib.check(lib.msw_flood_maps_launch(nrows, T, C.byref(g), C.byref(r), C.byref(it)))
    assert it.value >= 3 and nrows % (g.value * r.value) != 0
    assert nrows * 2 * T * 4 < 16 << 20
    host = make_rollout(nrows, T, seed=9)
    bufs = Buffers(nrows, 2, cuda)
    update(host.to(cuda), bufs, 0, T, 0, 0, nrows, THR4[:2])
    assert_maps(bufs, expected(host, THR4[:2]), 2, f"nrows={nrows}")


def carry_rollout():
    """T = 48 with, planted: a maximum of h tied across the 16 | 16 boundary (steps 15 and 16; the
    earlier keeps it), one tied across 47 | 48 and 5 | 43, rows wet only in steps 0..15 and 32..47."""
    host = make_rollout(300, 48, seed=21)
    host[0::5, 0, 15] = host[0::5, 0, 16] = 4.0
    host[1::5, 1, 4] = 5.0
    host[1::5, 1, 5] = -5.0
    host[2::5, 0, 46] = host[2::5, 0, 47] = 6.0
    host[3::5, 0, 16:32] = 0.0
    host[3::5, 0, :16] += 0.5
    host[3::5, 0, 32:] += 0.5
    return host


@pytest.mark.parametrize("split", [(1,) * 48, (16, 16, 16), (5, 43), (47, 1)], ids=["48x1", "16+16+16", "5+43", "47+1"])
@pytest.mark.parametrize("how", ["windows", "pieces"])
def test_carry_over_equals_one_shot(cuda, split, how):
    host = carry_rollout()
    dev = host.to(cuda)
    n, thr = host.shape[0] - 9, THR4[:3]
    want = expected(host[4:4 + n], thr)
    one = Buffers(n, 3, cuda)
    update(dev, one, 0, 48, 0, 4, n, thr)
    assert_maps(one, want, 3, "one shot")
    bufs = Buffers(n, 3, cuda)
    t0 = 0
    for c in split:
        if how == "windows":   # a window of the stored rollout
            update(dev, bufs, t0, c, t0, 4, n, thr, first=int(t0 == 0))
        else:                  # a rollout piece of its own, as rollout_chunks yields them
            update(dev[:, :, t0:t0 + c].contiguous(), bufs, 0, c, t0, 4, n, thr, first=int(t0 == 0))
        t0 += c
    assert_maps(bufs, want, 3, f"{how} {split}")


@pytest.mark.parametrize("T, split", fc.CARRY, ids=[f"T{T}-" + "+".join(map(str, p)) for T, p in fc.CARRY])
@pytest.mark.parametrize("how", ["windows", "pieces"])
def test_carry_over_across_parts_and_slabs(cuda, T, split, how):
    n, thr = fc.PERIOD + 8, THR4[:3]
    host = fc.planted_rollout(n + 9, T, 0, T, seed=T)
    dev = host.to(cuda)
    want = expected(host[4:4 + n], thr)
    one = Buffers(n, 3, cuda)
    update(dev, one, 0, T, 0, 4, n, thr)
    assert_maps(one, want, 3, "one shot")
    bufs = Buffers(n, 3, cuda)
    t0 = 0
    for c in split:
        if how == "windows":
            update(dev, bufs, t0, c, t0, 4, n, thr, first=int(t0 == 0))
        else:
            update(dev[:, :, t0:t0 + c].contiguous(), bufs, 0, c, t0, 4, n, thr, first=int(t0 == 0))
        t0 += c
    assert_maps(bufs, want, 3, f"{how} {split}")
    for k, v in bufs.view.items():      # and bit for bit the one-shot result, froude_max included
        assert torch.equal(v, one.view[k]), k


@pytest.mark.parametrize("subset", [("wet_steps",), ("h_max", "t_h_max"),
                                    tuple(k for k in MAP_NAMES if k not in ("vel_max", "froude_max"))],
                         ids=["wet_steps", "h_max+t_h_max", "no_velocity"])
def test_null_subsets(cuda, subset):
    host = carry_rollout()
    dev = host.to(cuda)
    n, thr = host.shape[0], THR4[:2]
    want = expected(host, thr)
    bufs = Buffers(n, 2, cuda, want=subset)
    assert set(bufs.view) == set(subset)
    update(dev, bufs, 0, 16, 0, 0, n, thr)
    update(dev, bufs, 16, 32, 16, 0, n, thr, first=0)
    assert_maps(bufs, want, 2, str(subset))
    # the Python interface with the same subset
    fm = FloodMaps(n, thresholds=thr, vel_eps=EPS, device=cuda, want=subset).update(dev, 0, 16).update(dev, 16)
    assert set(fm.maps) == set(subset)
    for k in subset:
        check_map(k, fm.maps[k], want, "FloodMaps")


@pytest.fixture(scope="module")
def engine(cuda):
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    m.engine = "hip"
    g = make_multiscale_mesh(**mesh_config("small"), T=48).to(cuda)
    whole = m.rollout(g, 48)
    torch.cuda.synchronize()
    return m, g, whole


def _same(u, v):
    if isinstance(u, dict):
        return u.keys() == v.keys() and all(_same(u[k], v[k]) for k in u)
    if isinstance(u, list):
        return len(u) == len(v) and all(_same(a, b) for a, b in zip(u, v))
    if not isinstance(u, torch.Tensor):
        return u == v
    if torch.is_floating_point(u):  # arrival_hours holds NaN where a cell was never wet
        u, v = torch.nan_to_num(u, nan=-7.0), torch.nan_to_num(v, nan=-7.0)
    return torch.equal(u, v)


def test_update_behind_rollout_on_a_side_stream(cuda, engine):
    from mswegnn.engine import plan_for
    m, g, whole = engine
    plan = plan_for(m, g)
    side = torch.cuda.Stream(cuda)
    fm = FloodMaps(g.x.shape[0], device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = plan.rollout(g.x, g.BC, g.node_BC, g.type_BC, 48)
        fm.update(out)       # enqueued directly behind the rollout: no synchronisation in between
    side.synchronize()
    assert torch.equal(out, whole)
    want = expected(whole.cpu(), (0.05, 0.3))
    for k in MAP_NAMES:
        check_map(k, fm.maps[k], want, "side stream")


@pytest.mark.parametrize("chunk", [16, 7])
def test_engine_chunked_rollout_and_maps(cuda, engine, chunk):
    from mswegnn.engine import plan_for
    m, g, whole = engine
    steps0 = plan_for(m, g).stats()["rollout_steps"]
    pieces = list(rollout_chunks(m, g, 48, chunk))
    assert plan_for(m, g).stats()["rollout_steps"] == steps0 + 48   # the HIP path ran them
    assert [t0 for t0, _ in pieces] == list(range(0, 48, chunk))
    assert torch.equal(torch.cat([p for _, p in pieces], -1), whole)
    res, kept = rollout_flood_maps(m, g, 48, chunk=chunk, keep_rollout=True, temporal_res=30, time_start=1)
    assert torch.equal(kept, whole)
    assert _same(res, flood_maps(whole, temporal_res=30, time_start=1))
    want = expected(whole.cpu(), (0.05, 0.3))
    for k in ("h_max", "t_q_max", "vel_max", "froude_max"):
        check_map(k, res[k], want, f"chunk={chunk}")


def test_engine_batch_one_result_per_simulation(cuda, engine):
    m = engine[0]
    gs = [wet_state(make_multiscale_mesh(**mesh_config("tiny"), T=32), seed=1),
          make_multiscale_mesh(n_coarse=3, num_scales=4, seed=5, T=32)]
    b = adapt_batch_training(collate(gs)).to(cuda)
    per_sim = rollout_flood_maps(m, b, 32, chunk=16, ranges=finest_ranges(b))
    assert len(per_sim) == 2
    assert _same(per_sim, flood_maps(m.rollout(b, 32), ranges=finest_ranges(b)))
    for g, res in zip(gs, per_sim):
        gd = g.to(cuda)
        alone = flood_maps(m.rollout(gd, 32), ranges=finest_ranges(gd))[0]
        assert _same(res, alone)
