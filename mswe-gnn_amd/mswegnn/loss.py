"""The training loss of the reference (training/loss.py:76-169) with the HIP loss kernels.

  get_mean_error        training/loss.py:8-23
  mask_on_water         training/loss.py:25-35
  loss variable scaler  training/loss.py:37-47
  get_multiscale_loss   training/loss.py:49-74
  loss_function         training/loss.py:76-118
  conservation_loss     training/loss.py:120-169
  get_inflow_volume     utils/dataset.py:577-591

``loss_function`` has the reference's signature and meaning.  ``training_step``
(training/train.py:125-145) calls it after each of its R curriculum rollout steps; with the
reference's default options (``only_where_water=True``) its boolean-mask selection is a
``nonzero`` and a device-to-host read per step.  On fp32 GPU tensors with at most 64 simulations
the call is a ``torch.autograd.Function`` over ``msw_train_loss_forward`` / ``_backward``
(csrc/loss.hip, include/mswegnn.h): two launches forward, one or two backward, fp64 sums in a
fixed order (bit-identical from call to call), no host synchronisation once ``ptr_list`` has read
``node_ptr``.  Everything else -- CPU tensors, other dtypes, more than 64 simulations -- runs
``torch_loss_function``, a torch composition that restates the reference op for op.

``MSWEGNN_FUSED_LOSS=1`` (read by ``models/__init__.py``, :mod:`mswegnn.hooks`) installs
``loss_function`` in place of the reference's inside ``training.train``.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from .rollout import is_batch, ptr_list

__all__ = ["loss_function", "torch_loss_function", "conservation_loss", "fine_ranges", "LOSS_CALLS"]

NUM_WATER_VARS = 2
LOSS_CALLS = [0]  # calls that ran the HIP kernels (tests check that the HIP path ran)


# ------------------------------------------------------------------ the torch composition
def _mean_error(diff, type_loss, nodes_dim=0):
    """loss.py:8-23"""
    if type_loss == 'RMSE':
        return torch.sqrt((diff ** 2).mean(nodes_dim))
    elif type_loss == 'MAE':
        return diff.abs().mean(nodes_dim)


def _mask_on_water(diff, water_axis=1):
    """loss.py:25-35"""
    return (diff != 0).any(water_axis)


def _has_node_ptr(data):
    return 'node_ptr' in data.keys()


def _multiscale_loss(diff, data, only_where_water, type_loss):
    """loss.py:49-74: the finest scale of every graph, optionally only the rows with water."""
    node_ptr = data.node_ptr
    if only_where_water:
        where = _mask_on_water(diff)
    else:
        where = torch.ones(diff.shape[0], device=diff.device).bool()
    if is_batch(data):
        rows = ptr_list(node_ptr)
        parts = [diff[rows[i][0]:rows[i][1]][where[rows[i][0]:rows[i][1]]] for i in range(data.num_graphs)]
        return _mean_error(torch.cat(parts), type_loss, 0)
    a, b = ptr_list(node_ptr)[:2]
    return _mean_error(diff[a:b][where[a:b]], type_loss, 0)


def conservation_loss(pred_WD, input_WD, data, BC):
    """loss.py:120-169: (predicted volume change of the finest scale - inflow volume - the ghost
    cells' share) / 1e6, divided by num_graphs for a batch."""
    assert pred_WD.shape == input_WD.shape, \
        f"Input or predictions have wrong dimensions ({pred_WD.shape} != {input_WD.shape})"
    delta_WD = pred_WD - input_WD
    assert delta_WD.dim() == 2, f"Input or predictions have wrong dimensions ({delta_WD.dim()})"
    assert BC.dim() == 1, f"Boundary conditions have wrong dimensions ({BC.dim()})"
    area = data.area if data.area.dim() == 2 else data.area.unsqueeze(1)
    if _has_node_ptr(data):
        if is_batch(data):
            rows = ptr_list(data.node_ptr)
            volume = torch.cat([(area * delta_WD)[rows[i][0]:rows[i][1]] for i in range(data.num_graphs)]).sum()
        else:
            a, b = ptr_list(data.node_ptr)[:2]
            volume = ((area * delta_WD)[a:b]).sum()
    else:
        volume = (area * delta_WD).sum()
    inflow = (BC * data.edge_BC_length).sum() * (60 * data.temporal_res)   # dataset.py:577-591
    correction = ((area * delta_WD)[data.node_BC]).sum()
    cons = (volume - inflow - correction) / 1e6
    if is_batch(data):
        cons = cons / data.num_graphs
    return cons


def torch_loss_function(preds, real, data, BC, type_loss='RMSE', only_where_water=False,
                        conservation=0, velocity_scaler=1):
    """loss.py:76-118 as a torch composition (any device and dtype)."""
    diff = preds - real
    if _has_node_ptr(data):
        loss = _multiscale_loss(diff, data, only_where_water, type_loss)
    else:
        if only_where_water:
            diff = diff[_mask_on_water(diff)]
        loss = _mean_error(diff, type_loss, 0)
    scaler = torch.ones(NUM_WATER_VARS)
    scaler[1::NUM_WATER_VARS] = velocity_scaler
    scaler = scaler.to(device=diff.device, dtype=loss.dtype)
    loss = torch.dot(loss, scaler) / scaler.sum()
    if conservation != 0:
        input_WD = data.x[:, -2::2]
        pred_WD = preds[:, 0::2]
        loss = loss + conservation * conservation_loss(pred_WD, input_WD, data, BC).abs()
    return loss


# ------------------------------------------------------------------ the HIP path
def fine_ranges(data, num_rows):
    """[(start, end)] of the finest scale of every graph (node_ptr through ptr_list: read from the
    device once per tensor), or [(0, N)] without node_ptr."""
    if not _has_node_ptr(data):
        return [(0, int(num_rows))]
    rows = ptr_list(data.node_ptr)
    if is_batch(data):
        return [(int(rows[i][0]), int(rows[i][1])) for i in range(data.num_graphs)]
    return [(int(rows[0]), int(rows[1]))]


def _ranges_ok(ranges, num_rows):
    at = 0
    for s, e in ranges:
        if s < at or e < s or e > num_rows:
            return False
        at = e
    return 1 <= len(ranges) <= L.MAX_LOSS_RANGES


def _stream(dev):
    from .engine import _raw_stream
    return C.c_void_p(_raw_stream(dev.index or 0))


def make_desc(num_rows, ranges, type_loss, only_where_water, velocity_scaler, conservation=0.0, num_graphs=1,
              seconds_per_step=0.0, area=None, input_h=None, input_h_stride=1, node_bc=None, bc=None,
              edge_bc_length=None, n_bc=0):
    """msw_train_loss_desc from Python values; the pointers are data_ptr() integers or None."""
    d = L.MswTrainLossDesc()
    d.num_rows = int(num_rows)
    d.num_ranges = len(ranges)
    d.type_loss = L.LOSS_TYPE.get(type_loss, -1) if isinstance(type_loss, str) else int(type_loss)
    for i, (s, e) in enumerate(ranges[:L.MAX_LOSS_RANGES]):
        d.ranges[i][0], d.ranges[i][1] = int(s), int(e)
    d.only_where_water = int(bool(only_where_water))
    d.num_graphs = int(num_graphs)
    d.velocity_scaler = float(velocity_scaler)
    d.conservation = float(conservation)
    d.seconds_per_step = float(seconds_per_step)
    d.area, d.input_h, d.input_h_stride = area, input_h, int(input_h_stride)
    d.node_bc, d.bc, d.edge_bc_length, d.n_bc = node_bc, bc, edge_bc_length, int(n_bc)
    return d


def workspace(desc):
    n = C.c_int64(0)
    L.check(L.lib().msw_train_loss_workspace(C.byref(desc), C.byref(n)))
    return int(n.value)


def launch(total_rows):
    """(grid, rows_per_wg, iters) of the forward's partial-sum launch (msw_train_loss_launch)."""
    g, r, i = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    L.check(L.lib().msw_train_loss_launch(int(total_rows), C.byref(g), C.byref(r), C.byref(i)))
    return g.value, r.value, i.value


class _LossFunction(torch.autograd.Function):
    """opts: (ranges, type_loss, only_where_water, velocity_scaler, conservation, num_graphs,
    seconds_per_step); cons: None or (area, node_bc, bc, edge_bc_length) device tensors."""

    @staticmethod
    def forward(ctx, opts, cons, preds, real, input_h):
        dev = preds.device
        preds, real = preds.contiguous(), real.contiguous()
        ranges, type_loss, mask, vs, c, G, seconds = opts
        kw = {}
        if cons is not None:
            area, node_bc, bc, length = cons
            kw = dict(conservation=c, num_graphs=G, seconds_per_step=seconds, area=area.data_ptr(),
                      input_h=input_h.data_ptr(), input_h_stride=input_h.stride(0) if input_h.shape[0] > 1 else 1,
                      node_bc=node_bc.data_ptr() if node_bc.numel() else None,
                      bc=bc.data_ptr() if bc.numel() else None,
                      edge_bc_length=length.data_ptr() if length.numel() else None, n_bc=node_bc.numel())
        d = make_desc(preds.shape[0], ranges, type_loss, mask, vs, **kw)
        scratch = torch.empty(workspace(d), device=dev, dtype=torch.float64)
        record = torch.empty(L.TRAIN_LOSS_RECORD, device=dev, dtype=torch.float64)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):  # the kernels launch on the current device
            L.check(L.lib().msw_train_loss_forward(C.byref(d), preds.data_ptr(), real.data_ptr(), scratch.data_ptr(),
                                                   loss.data_ptr(), record.data_ptr(), _stream(dev)))
        # the backward does not read input_h (training_step overwrites data.x in place before it runs)
        ctx.desc, ctx.cons = d, cons
        ctx.save_for_backward(preds, real, record)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        preds, real, record = ctx.saved_tensors
        dev = preds.device
        gout = gout.contiguous().to(torch.float32)
        gp = torch.empty_like(preds)
        want_in = ctx.cons is not None and ctx.needs_input_grad[4]
        gin = torch.empty(preds.shape[0], device=dev, dtype=torch.float32) if want_in else None
        with torch.cuda.device(dev):  # the kernels launch on the current device
            L.check(L.lib().msw_train_loss_backward(C.byref(ctx.desc), preds.data_ptr(), real.data_ptr(),
                                                    record.data_ptr(), gout.data_ptr(), gp.data_ptr(),
                                                    gin.data_ptr() if gin is not None else None, _stream(dev)))
        return None, None, gp, None, gin  # targets that require grad take the torch composition


def _hip_args(preds, real, data, BC, type_loss, only_where_water, conservation, velocity_scaler):
    """The HIP call's arguments, or None where the torch composition has to run."""
    if not (torch.is_tensor(preds) and torch.is_tensor(real) and preds.is_cuda and real.is_cuda):
        return None
    if torch.is_autocast_enabled():  # the kernels compute in fp32, as the other training functions
        if preds.dtype in (torch.float16, torch.bfloat16):
            preds = preds.float()
        if real.dtype in (torch.float16, torch.bfloat16):
            real = real.float()
    if (preds.dtype != torch.float32 or real.dtype != torch.float32 or preds.dim() != 2
            or preds.shape[1] != NUM_WATER_VARS or real.shape != preds.shape or type_loss not in L.LOSS_TYPE
            or real.requires_grad):
        return None
    N = int(preds.shape[0])
    ranges = fine_ranges(data, N)
    if not _ranges_ok(ranges, N):
        return None
    cons, input_h, G, seconds = None, None, 1, 0.0
    if conservation != 0:
        x, area = data.x, data.area
        if not (torch.is_tensor(BC) and BC.dim() == 1 and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
                and x.shape[0] == N and area.is_cuda and area.numel() == N):
            return None
        input_h = x[:, -2]
        node_bc = data.node_BC.reshape(-1).long().contiguous()
        length = data.edge_BC_length
        if not torch.is_tensor(length):
            length = torch.as_tensor(length, dtype=torch.float32, device=preds.device)
        try:
            length = torch.broadcast_to(length.to(device=preds.device, dtype=torch.float32), BC.shape).contiguous()
        except RuntimeError:
            return None
        if node_bc.numel() != BC.numel():
            return None
        tres = data.temporal_res
        tres = ptr_list(tres) if torch.is_tensor(tres) else tres
        seconds = 60.0 * float(tres)
        G = int(data.num_graphs) if is_batch(data) else 1
        cons = (area.reshape(-1).float().contiguous(), node_bc, BC.detach().float().contiguous(), length)
    opts = (ranges, type_loss, bool(only_where_water), float(velocity_scaler), float(conservation), G, seconds)
    return opts, cons, preds, real, input_h


def loss_function(preds, real, data, BC, type_loss='RMSE', only_where_water=False,
                  conservation=0, velocity_scaler=1):
    """The reference's loss_function (training/loss.py:76-118): RMSE or MAE over the finest
    scale of every graph, optionally only where there is water, the velocity column weighted by
    ``velocity_scaler``, plus ``conservation`` x |mass-conservation residual|."""
    args = _hip_args(preds, real, data, BC, type_loss, only_where_water, conservation, velocity_scaler)
    if args is None:
        return torch_loss_function(preds, real, data, BC, type_loss, only_where_water, conservation,
                                   velocity_scaler)
    opts, cons, preds, real, input_h = args
    LOSS_CALLS[0] += 1
    if input_h is None:
        input_h = preds.new_empty(0)
    return _LossFunction.apply(opts, cons, preds, real, input_h)
