"""Autograd through the HIP training kernels.

``swegnn_apply(layer, x_s, x_d, edge_index, edge_attr)`` runs one ``SWEGNN`` processor
(models/gnn.py:387-445) as a ``torch.autograd.Function`` whose forward and backward are the
gfx950 kernels of ``csrc/train.hip`` behind the C ABI (``msw_swegnn_train_*``,
include/mswegnn.h): every parameter and input gradient the reference's ``training_step``
(training/train.py:125-145) back-propagates through the layer is computed by HIP kernels --
MFMA GEMMs for the edge-MLP and filter layers (split-K weight gradients), CSR pulls by
destination and by source for the hop's transpose, no atomics.  torch only allocates the
buffers (saved state, scratch, gradients) and orders the work on its current stream.

``mlp_apply(seq, x)`` does the same for a make_mlp Sequential (models/models.py:121-146: the
edge / node encoders and the node decoder) over ``msw_mlp_train_*``.

``pool_apply(x, pool_edges)`` is MSGNN's mean pooling (models/gnn.py:242-257) over
``msw_pool_mean_*``: CSR pulls by coarse node (forward) and by fine node (backward), no
atomics, so the whole training forward / backward is deterministic.

``SWEGNN.forward``, the models' encoder / decoder calls and MSGNN's pooling (models/gnn.py of
this package) route here on a GPU with autograd enabled; the scale selections, skip sums and
the output mask stay elementwise torch ops.  The loss that ``training_step`` evaluates on the
model's output is built too: :mod:`mswegnn.loss` over ``msw_train_loss_*`` (csrc/loss.hip),
opt-in through ``MSWEGNN_FUSED_LOSS=1``.
"""
from __future__ import annotations

import ctypes as C
import weakref
from collections import OrderedDict

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib as L
from .engine import _act_code, _raw_stream

__all__ = ["swegnn_apply", "supported", "graph_csr", "mlp_apply", "mlp_supported", "pool_apply", "pool_supported",
           "clear_caches"]

_CSR_CACHE = OrderedDict()
_CSR_KEEP = 32
MLP_CALLS = [0]  # mlp_apply / pool_apply / swegnn_apply calls (tests check that the HIP path ran)
POOL_CALLS = [0]
SWEGNN_CALLS = [0]
# Diagnostics (tests/: the branch-following float64 yardstick).  A list here receives, per HIP
# training-forward call in call order, the discrete decisions the kernels took: the side of
# every activation kink (pre-activation > 0) of each MLP layer and, for SWEGNN, the hop
# predicate out.sum(1) != 0 of every hop (gnn.py:408) -- read back from the saved buffer.
RECORD = None


def _al(n):
    return (n + 63) // 64 * 64  # csrc/train.hip al(): every slot starts on a 64-float boundary


# The saved buffers, restated from csrc/train.hip as float offsets (tests/test_host_cpu.py holds
# each "end" against msw_*_train_workspace's saved_floats).
def _stack_offsets(d, rows, o, keep_last):
    """stack_layout_of: pre[0..L), then post[0..L) -- without the last layer's output unless
    keep_last -- from offset o."""
    off = {"pre": [], "post": []}
    for name, n in (("pre", d.n_layers), ("post", d.n_layers if keep_last else d.n_layers - 1)):
        for l in range(n):
            off[name].append(o)
            o += _al(rows * d.width[l + 1])
    off["end"] = o
    return off


def _mlp_offsets(d):
    """msw_mlp_train_forward's saved buffer (mlp_layout_of): the stack alone."""
    return _stack_offsets(d, d.rows, 0, False)


def _swegnn_offsets(d):
    """msw_swegnn_train_forward's saved buffer (layout_of): X0, the edge MLP's stack, then s, nrm,
    outk, agg, nz."""
    E, N, F, K = d.num_edges, d.num_nodes, d.F, d.K
    off = _stack_offsets(d, E, _al(E * d.width[0]), True)
    o = off["end"]
    for name, n in (("s", E * F), ("nrm", E), ("outk", (K + 1) * N * F), ("agg", K * N * F), ("nz", K * N)):
        off[name] = o
        o += _al(n)
    off["X0"], off["end"] = 0, o
    return off


def _pre_signs(d, saved, rows, off):
    return [saved[o:o + rows * d.width[l + 1]].view(rows, d.width[l + 1]) > 0 for l, o in enumerate(off["pre"])]


def _swegnn_decisions(d, saved):
    """-> {pre: [E x w(l+1) bool], nz: [K x N bool]} read from the saved buffer."""
    off, K, N = _swegnn_offsets(d), d.K, d.num_nodes
    nz = saved[off["nz"]:off["nz"] + K * N].view(torch.int32).view(K, N) != 0
    return {"kind": "swegnn", "pre": _pre_signs(d, saved, d.num_edges, off), "nz": [nz[k] for k in range(K)]}


def _mlp_decisions(d, saved):
    return {"kind": "mlp", "pre": _pre_signs(d, saved, d.rows, _mlp_offsets(d))}


class GraphCSR:
    """row / col (int32) and the CSRs by destination (col) and by source (row) of one
    edge_index on the GPU; each node's edges in reference (edge_index) order."""

    def __init__(self, edge_index, num_nodes):
        ei = edge_index.to(torch.int64)
        dev = ei.device
        self.num_nodes = int(num_nodes)
        self.num_edges = int(ei.shape[1])
        self.row = ei[0].to(torch.int32).contiguous()
        self.col = ei[1].to(torch.int32).contiguous()

        def csr(key):
            order = torch.sort(key, stable=True).indices.to(torch.int32).contiguous()
            cnt = torch.bincount(key, minlength=self.num_nodes)
            ptr = torch.zeros(self.num_nodes + 1, dtype=torch.int64, device=dev)
            ptr[1:] = torch.cumsum(cnt, 0)
            return ptr.to(torch.int32).contiguous(), order
        self.in_ptr, self.in_edge = csr(ei[1])
        self.out_ptr, self.out_edge = csr(ei[0])


def _drop_csr(key):
    """Forget one cached GraphCSR and every descriptor template bound to it; its owner's
    finalizer is detached (one finalizer per live entry: a graph re-cached every epoch does not
    pile them up, and a stale one can never drop a newer entry under the same key)."""
    ent = _CSR_CACHE.pop(key, None)
    if ent is not None:
        ent[2].detach()
        # a snapshot: a finalizer fired by the cyclic GC may call back into here
        for k in [k for k, m in list(_META_CACHE.items()) if getattr(m, "csr", None) is ent[1]]:
            _META_CACHE.pop(k, None)


def graph_csr(edge_index, num_nodes):
    """Cached GraphCSR, keyed by the index tensor's address, layout and in-place version.  The
    entry holds only a weak reference to the storage owner (the tensor, or the base of a
    slice such as MSGNN's per-scale ``edge_index[:, a:b]``) and is dropped, with the
    descriptors bound to it, when that owner is collected: a training loop over many batches
    keeps no previous batch's graph (or its GPU CSR) alive."""
    key = (edge_index.data_ptr(), tuple(edge_index.shape), tuple(edge_index.stride()), edge_index._version,
           int(num_nodes), str(edge_index.device))
    owner = edge_index._base if edge_index._base is not None else edge_index
    hit = _CSR_CACHE.get(key)
    if hit is not None and hit[0]() is owner:
        _CSR_CACHE.move_to_end(key)
        return hit[1]
    _drop_csr(key)
    g = GraphCSR(edge_index, num_nodes)
    _CSR_CACHE[key] = (weakref.ref(owner), g, weakref.finalize(owner, _drop_csr, key))
    while len(_CSR_CACHE) > _CSR_KEEP:
        _drop_csr(next(iter(_CSR_CACHE)))
    return g


def clear_caches():
    """Drop every cached CSR and descriptor template (their GPU arrays are freed)."""
    for ent in list(_CSR_CACHE.values()):
        ent[2].detach()
    _CSR_CACHE.clear()
    _META_CACHE.clear()


def _mlp_layers(seq):
    """make_mlp Sequential -> [(Linear, activation module or None)]; None if unsupported."""
    layers = []
    for m in seq:
        if isinstance(m, nn.Linear):
            layers.append([m, None])
        elif isinstance(m, nn.Dropout):
            if m.p > 0 and m.training:
                return None
        elif isinstance(m, nn.LayerNorm):
            return None
        elif layers:
            layers[-1][1] = m
        else:
            return None
    if not 1 <= len(layers) <= L.MAX_MLP_LAYERS:
        return None
    for lin, act in layers:
        try:
            _act_code(act)
        except NotImplementedError:
            return None
    return layers


def supported(layer, x_s, x_d, edge_attr):
    """The HIP training path implements this layer call (else the torch path runs): fp32 GPU
    tensors, static and dynamic node features of one width F over the same rows (the kernels'
    edge-MLP input is [x_s(row), x_s(col), x_d(row), x_d(col), e] = 4F + ef wide), no double
    backward (the kernels' backward is not itself differentiable)."""
    if not (x_d.is_cuda and x_s.is_cuda) or x_d.dtype != torch.float32 or x_s.dtype != torch.float32:
        return False
    if x_s.dim() != 2 or x_d.dim() != 2 or x_s.shape != x_d.shape:
        return False
    if layer.K < 1 or layer.K > L.MAX_HOPS or _mlp_layers(layer.edge_mlp) is None:
        return False
    ef = int(layer.edge_features) if layer.edge_features > 0 else 0
    if _mlp_layers(layer.edge_mlp)[0][0].in_features != 4 * x_d.shape[1] + ef:
        return False
    if layer.edge_features > 0 and (edge_attr is None or edge_attr.dtype != torch.float32):
        return False
    return all(p.dtype == torch.float32 and p.is_cuda for p in layer.parameters())


def _slots(mods, layer=None):
    """(descriptor field, index, parameter) of every parameter a descriptor binds, in binding
    order = the order of the Functions' *params: per Linear of the module sequence `mods` its
    weight, its bias if it has one and the slope of a PReLU behind it, then `layer`'s K + 1 filter
    matrices if it has them.  The one walk: descriptors, gradient structs and the cache
    validation all go by it."""
    i = -1
    for m in mods:
        if isinstance(m, nn.Linear):
            i += 1
            yield "weight", i, m.weight
            if m.bias is not None:
                yield "bias", i, m.bias
        elif isinstance(m, nn.PReLU):
            yield "slope", i, m.weight
    if layer is not None and layer.with_filter_matrix:
        for k, f in enumerate(layer.filter_matrix):
            yield "filter", k, f.weight


def _param_list(layer=None, seq=None):
    """The parameter objects a descriptor binds, in its order (cache validation)."""
    return [p for _, _, p in _slots(layer.edge_mlp if layer is not None else seq, layer)]


class _StackMeta:
    """One make_mlp stack described once, from _mlp_layers(seq): the width / act fill of either
    descriptor type, the parameter objects in binding order, their binding into the descriptor
    and of their gradients into either grads struct, and the workspace sizes.  With the
    descriptor `desc` it is everything but the tensors autograd tracks: the template of one
    call."""

    def __init__(self, layers, desc, workspace, layer=None):
        self.layers, self.desc, self.workspace, self.ws = layers, desc, workspace, None
        desc.n_layers = len(layers)
        desc.width[0] = layers[0][0].in_features
        for i, (lin, act) in enumerate(layers):
            desc.width[i + 1] = lin.out_features
            desc.act[i] = _act_code(act)
        slots = list(_slots((m for pair in layers for m in pair), layer))
        self.slots = [(field, i) for field, i, _ in slots]
        self.params = [p for _, _, p in slots]

    def bind(self, params):
        """Point the descriptor at the (contiguous) parameter tensors of this call."""
        for (field, i), p in zip(self.slots, params):
            getattr(self.desc, field)[i] = p.data_ptr()
        return self.desc

    def bind_grads(self, g, grads):
        """Point the grads struct at the gradient tensors (None: not wanted) of this call."""
        for (field, i), t in zip(self.slots, grads):
            getattr(g, "d_" + field)[i] = t.data_ptr() if t is not None else None

    def sizes(self):
        """(saved, scratch) floats: they depend on the descriptor's sizes only, asked once."""
        if self.ws is None:
            s, t = C.c_int64(), C.c_int64()
            L.check(getattr(L.lib(), self.workspace)(C.byref(self.desc), C.byref(s), C.byref(t)))
            self.ws = int(s.value), int(t.value)
        return self.ws


class _Meta(_StackMeta):
    """A SWEGNN layer's call: its edge MLP's stack, the graph, the flags and the filters."""

    def __init__(self, layer, layers, csr, F, ef):
        self.layer, self.csr, self.F, self.ef = layer, csr, F, ef
        d = L.MswSwegnnTrainDesc()
        d.num_nodes, d.num_edges = csr.num_nodes, csr.num_edges
        d.F, d.edge_features, d.K = F, ef, layer.K
        d.normalize = int(bool(layer.normalize))
        d.with_filter_matrix = int(bool(layer.with_filter_matrix))
        d.with_gradient = int(bool(layer.with_gradient))
        d.upwind_mode = int(bool(layer.upwind_mode))
        for name in ("row", "col", "in_ptr", "in_edge", "out_ptr", "out_edge"):
            setattr(d, name, getattr(csr, name).data_ptr())
        super().__init__(layers, d, "msw_swegnn_train_workspace", layer)


class _MlpMeta(_StackMeta):
    def __init__(self, layers, rows):
        d = L.MswMlpTrainDesc()
        d.rows = rows
        super().__init__(layers, d, "msw_mlp_train_workspace")


_META_CACHE = OrderedDict()
_META_KEEP = 64


def _cached_meta(key, params_now, make):
    """Descriptor templates reused across calls (their ctypes structs cost more host time than
    the launches): keyed by the module and graph; valid while the module holds the same
    parameter objects (a replaced Parameter rebuilds it)."""
    hit = _META_CACHE.get(key)
    if hit is not None and len(hit.params) == len(params_now) and all(a is b for a, b in zip(hit.params, params_now)):
        _META_CACHE.move_to_end(key)
        return hit
    meta = make()
    _META_CACHE[key] = meta
    while len(_META_CACHE) > _META_KEEP:
        _META_CACHE.popitem(last=False)
    return meta


class _SwegnnFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, x_s, x_d, edge_attr, *params):
        dev = x_d.device
        x_s, x_d = x_s.contiguous(), x_d.contiguous()
        ea = edge_attr.contiguous() if meta.ef > 0 else None
        params = [p.contiguous() for p in params]
        d = meta.bind(params)
        n_saved, _ = meta.sizes()
        saved = torch.empty(n_saved, device=dev, dtype=torch.float32)
        out = torch.empty(meta.csr.num_nodes, meta.F, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):  # the kernels launch on the current device
            L.check(L.lib().msw_swegnn_train_forward(C.byref(d), x_s.data_ptr(), x_d.data_ptr(),
                                                     ea.data_ptr() if ea is not None else None,
                                                     saved.data_ptr(), out.data_ptr(),
                                                     C.c_void_p(_raw_stream(dev.index or 0))))
        if RECORD is not None:
            RECORD.append(_swegnn_decisions(d, saved))
        ctx.meta = meta
        ctx.has_ea = edge_attr is not None
        ctx.save_for_backward(x_s, x_d, ea if ea is not None else torch.empty(0, device=dev), saved, *params)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        meta = ctx.meta
        x_s, x_d, ea, saved, *params = ctx.saved_tensors
        dev = x_d.device
        gout = gout.contiguous().to(torch.float32)
        d = meta.bind(params)
        _, n_scratch = meta.sizes()
        scratch = torch.empty(n_scratch, device=dev, dtype=torch.float32)
        g = L.MswSwegnnGrads()
        dxs = torch.empty_like(x_s) if ctx.needs_input_grad[1] else None
        dxd = torch.empty_like(x_d)
        dea = torch.empty_like(ea) if meta.ef > 0 and ctx.needs_input_grad[3] else None
        g.d_x_s = dxs.data_ptr() if dxs is not None else None
        g.d_x_d = dxd.data_ptr()
        g.d_edge_attr = dea.data_ptr() if dea is not None else None
        dps = [torch.empty_like(p) if ctx.needs_input_grad[4 + i] else None for i, p in enumerate(params)]
        meta.bind_grads(g, dps)
        with torch.cuda.device(dev):  # the kernels launch on the current device
            L.check(L.lib().msw_swegnn_train_backward(C.byref(d), x_s.data_ptr(), x_d.data_ptr(),
                                                      ea.data_ptr() if meta.ef > 0 else None, saved.data_ptr(),
                                                      gout.data_ptr(), C.byref(g), scratch.data_ptr(),
                                                      C.c_void_p(_raw_stream(dev.index or 0))))
        return (None, dxs, dxd, dea if ctx.has_ea else None, *dps)


def swegnn_apply(layer, x_s, x_d, edge_index, edge_attr=None):
    """SWEGNN.forward of `layer` on the HIP training kernels (differentiable)."""
    F = int(x_d.shape[1])
    ef = int(layer.edge_features) if layer.edge_features > 0 else 0
    csr = graph_csr(edge_index, x_d.shape[0])
    key = ("swegnn", id(layer), id(csr), F, ef, layer.K, bool(layer.normalize), bool(layer.with_filter_matrix),
           bool(layer.with_gradient), bool(layer.upwind_mode))
    meta = _cached_meta(key, _param_list(layer),
                        lambda: _Meta(layer, _mlp_layers(layer.edge_mlp), csr, F, ef))
    if ef > 0 and edge_attr.dim() == 1:
        edge_attr = edge_attr.unsqueeze(1)
    SWEGNN_CALLS[0] += 1
    return _SwegnnFunction.apply(meta, x_s, x_d, edge_attr if ef > 0 else None, *meta.params)


def mlp_supported(seq, x):
    """The HIP training path implements this make_mlp call (else the module runs)."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        return False
    layers = _mlp_layers(seq)
    if layers is None or layers[0][0].in_features != x.shape[1]:
        return False
    return all(p.dtype == torch.float32 and p.is_cuda for p in seq.parameters())


class _MlpFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, x, *params):
        dev = x.device
        x = x.contiguous()
        params = [p.contiguous() for p in params]
        d = meta.bind(params)
        n_saved, _ = meta.sizes()
        saved = torch.empty(max(n_saved, 1), device=dev, dtype=torch.float32)
        out = torch.empty(x.shape[0], meta.layers[-1][0].out_features, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):  # the kernels launch on the current device
            L.check(L.lib().msw_mlp_train_forward(C.byref(d), x.data_ptr(), saved.data_ptr(), out.data_ptr(),
                                                  C.c_void_p(_raw_stream(dev.index or 0))))
        if RECORD is not None:
            RECORD.append(_mlp_decisions(d, saved))
        ctx.meta = meta
        ctx.save_for_backward(x, saved, *params)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        meta = ctx.meta
        x, saved, *params = ctx.saved_tensors
        dev = x.device
        gout = gout.contiguous().to(torch.float32)
        d = meta.bind(params)
        _, n_scratch = meta.sizes()
        scratch = torch.empty(max(n_scratch, 1), device=dev, dtype=torch.float32)
        g = L.MswMlpGrads()
        dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        g.d_x = dx.data_ptr() if dx is not None else None
        dps = [torch.empty_like(p) if ctx.needs_input_grad[2 + i] else None for i, p in enumerate(params)]
        meta.bind_grads(g, dps)
        with torch.cuda.device(dev):  # the kernels launch on the current device
            L.check(L.lib().msw_mlp_train_backward(C.byref(d), x.data_ptr(), saved.data_ptr(), gout.data_ptr(),
                                                   C.byref(g), scratch.data_ptr(),
                                                   C.c_void_p(_raw_stream(dev.index or 0))))
        if dx is not None and x.shape[0] == 0:
            dx.zero_()
        return (None, dx, *dps)


def mlp_apply(seq, x):
    """make_mlp `seq` applied to x [rows][in] on the HIP training kernels (differentiable)."""
    rows = int(x.shape[0])
    meta = _cached_meta(("mlp", id(seq), rows), _param_list(seq=seq), lambda: _MlpMeta(_mlp_layers(seq), rows))
    MLP_CALLS[0] += 1
    return _MlpFunction.apply(meta, x, *meta.params)


class _PoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, csr, x):
        x = x.contiguous()
        out = torch.empty_like(x)
        dev = x.device
        with torch.cuda.device(dev):  # the kernels launch on the current device
            L.check(L.lib().msw_pool_mean_forward(csr.num_nodes, int(x.shape[1]), csr.col.data_ptr(),
                                                  csr.out_ptr.data_ptr(), csr.out_edge.data_ptr(), x.data_ptr(),
                                                  out.data_ptr(), C.c_void_p(_raw_stream(dev.index or 0))))
        ctx.csr = csr
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        csr = ctx.csr
        gout = gout.contiguous().to(torch.float32)
        dx = torch.empty_like(gout)
        dev = gout.device
        with torch.cuda.device(dev):  # the kernels launch on the current device
            L.check(L.lib().msw_pool_mean_backward(csr.num_nodes, int(gout.shape[1]), csr.row.data_ptr(),
                                                   csr.out_ptr.data_ptr(), csr.in_ptr.data_ptr(),
                                                   csr.in_edge.data_ptr(), gout.data_ptr(), dx.data_ptr(),
                                                   C.c_void_p(_raw_stream(dev.index or 0))))
        return None, dx


def pool_supported(x, pool_edges):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and pool_edges.is_cuda
            and pool_edges.dim() == 2 and pool_edges.shape[0] == 2)


def pool_apply(x, pool_edges):
    """Mean pooling of x [N][F] over pool_edges [2][E] = (coarse, fine) rows (a slice of
    intra_mesh_edge_index, gnn.py:310) on the HIP kernels (differentiable)."""
    POOL_CALLS[0] += 1
    return _PoolFunction.apply(graph_csr(pool_edges, x.shape[0]), x)
