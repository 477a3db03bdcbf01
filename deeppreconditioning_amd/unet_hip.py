"""The HIP forward of `PreconditionerSparseUNet` (inference): `dpcg_unet_*` in include/dpcg.h, csrc/dpcg_unet.hip.

A plan per sparsity pattern holds the five site sets S0 .. S4 and every rulebook (built on the device, no sort, no atomics);
the forward runs the 17 layers as gathered GEMMs on the fp32 matrix cores with bias, LeakyReLU and the skip adds fused, and
writes channel 0 of the output into a lower-triangular CSR (`output.lower_csr`, what `lower_factor_csr` / `LLtMultiply`
take).  `PreconditionerSparseUNet.forward` takes this path under the conditions of `PreconditionerNet`'s (CUDA, fp32
features, int32 indices, no autograd, `DPCG_CNN_TORCH` not 1) when the module has the reference's structure; anything else
runs the torch restatement in extras_unet.py unchanged."""

from __future__ import annotations

import ctypes as C
import os

import torch
from torch import nn

from .utils import SparseBatch

# module names in the order of the C ABI's layers, and the kind of each 3 x 3 layer
LAYERS = ("enc1", "down1", "enc2", "down2", "enc3", "down3", "enc4", "bottleneck",
          "up3", "dec3", "up2", "dec2", "up1", "dec1", "up0", "dec0", "out_conv")
_DOWN_OF_UP = {"up3": "bottleneck", "up2": "down3", "up1": "down2", "up0": "down1"}
LEVELS = 5


class _PlanCache(dict):
    """The module's plans by pattern.  Device handles do not copy: a deep copy or a pickle of the module starts empty."""

    def __deepcopy__(self, memo):
        return _PlanCache()

    def __reduce__(self):
        return (_PlanCache, ())


class _UnetPlan:
    """Owner of a `dpcg_unet_plan_t` (levels + rulebooks for ONE sparsity pattern).  `rebuild` re-targets it at another
    pattern reusing its device memory (dpcg_unet_plan_rebuild)."""

    def __init__(self, indices: torch.Tensor, batch: int, shape):
        self.handle = C.c_void_p()
        self._build(indices, batch, shape, create=True)

    def rebuild(self, indices: torch.Tensor, batch: int, shape) -> None:
        self._build(indices, batch, shape, create=False)

    def _build(self, indices, batch, shape, create: bool) -> None:
        from . import _lib as L
        self._L = L
        self.indices = indices                         # kept alive: the cache key is its storage
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        args = (int(batch), int(shape[0]), int(shape[1]), int(indices.shape[0]), C.c_void_p(indices.data_ptr()), stream)
        if create:
            L.check(L.lib().dpcg_unet_plan_create(C.byref(self.handle), *args))
        else:
            L.check(L.lib().dpcg_unet_plan_rebuild(self.handle, *args))
        self.levels = [self.info(lv) for lv in range(LEVELS)]
        self.sites, self.nnz_lower, self.batch = self.levels[0]["sites"], self.levels[0]["nnz_lower"], int(batch)
        self.out_shape = list(self.levels[0]["shape"])
        dev = indices.device
        # fresh output arrays per pattern (results of an earlier pattern that the caller still holds stay valid)
        self.out_indices = torch.empty((self.sites, 3), dtype=torch.int32, device=dev)
        self.lower_rowptr = torch.empty(self.batch * self.out_shape[0] + 1, dtype=torch.int32, device=dev)
        self.lower_col = torch.empty(self.nnz_lower, dtype=torch.int32, device=dev)
        L.check(L.lib().dpcg_unet_plan_output(self.handle, C.c_void_p(self.out_indices.data_ptr()),
                                              C.c_void_p(self.lower_rowptr.data_ptr()), C.c_void_p(self.lower_col.data_ptr()),
                                              stream))

    def info(self, level: int) -> dict:
        L = self._L
        sites, h, w, nl = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib().dpcg_unet_plan_info(self.handle, level, C.byref(sites), C.byref(h), C.byref(w), C.byref(nl)))
        return {"sites": sites.value, "shape": [h.value, w.value], "nnz_lower": nl.value}

    def level_indices(self, level: int) -> torch.Tensor:
        """(sites, 3) int32 indices of level `level` (0 = the input sites, 4 = the bottleneck's), sorted."""
        L = self._L
        out = torch.empty((self.levels[level]["sites"], 3), dtype=torch.int32, device=self.indices.device)
        L.check(L.lib().dpcg_unet_plan_level_indices(self.handle, level, C.c_void_p(out.data_ptr()),
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out

    def close(self):
        if self.handle is not None and self.handle.value:
            self._L.lib().dpcg_unet_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def _unet_layers(net):
    """[(conv, LeakyReLU or None)] in the ABI's order, or None when the module is not the reference's structure."""
    from .extras_unet import SparseInverseConv2d, SubMConv2d
    from .model import SparseConv2d
    out = []
    for name in LAYERS:
        seq = getattr(net, name, None)
        if not isinstance(seq, nn.Sequential):
            return None
        mods = list(seq)
        last = name == "out_conv"
        if len(mods) != (1 if last else 2):
            return None
        conv, act = mods[0], (None if last else mods[1])
        if not last and type(act) is not nn.LeakyReLU:
            return None
        if last or name.startswith(("enc", "dec")):
            ks, pad = ((1, 1), (0, 0)) if last else ((3, 3), (1, 1))
            if type(conv) is not SubMConv2d or tuple(conv.kernel_size) != ks or tuple(conv.padding) != pad:
                return None
        elif name.startswith("up"):
            down = getattr(net, _DOWN_OF_UP[name])[0]
            if (type(conv) is not SparseInverseConv2d or tuple(conv.kernel_size) != (3, 3)
                    or conv.indice_key != getattr(down, "indice_key", None)):
                return None
        else:
            if (type(conv) is not SparseConv2d or tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (2, 2)
                    or tuple(conv.padding) != (1, 1)):
                return None
        if conv.weight.dtype != torch.float32 or (conv.bias is not None and conv.bias.dtype != torch.float32):
            return None
        out.append((conv, act))
    return out


def hip_unet_applies(net, t: SparseBatch) -> bool:
    """The conditions of `PreconditionerNet`'s HIP path, plus the reference's U-Net structure."""
    if os.environ.get("DPCG_CNN_TORCH") == "1" or torch.is_grad_enabled():
        return False
    if not (t.features.is_cuda and t.features.dtype == torch.float32 and t.indices.dtype == torch.int32):
        return False
    layers = _unet_layers(net)
    return layers is not None and all(c.weight.is_cuda for c, _ in layers)


def _plan_for(net, t: SparseBatch, _sorted_once: bool = False):
    """(plan, features, t) for the pattern of `t`: the cached plan, a new one, or the oldest of two rebuilt.  Sites in another
    order than (batch, row, col) are sorted once (the returned t is then the sorted batch)."""
    from . import _lib as L
    cache = net.__dict__.setdefault("_hip_unet_plans", _PlanCache())
    indices = t.indices.contiguous()
    feats = t.features.contiguous()
    # (tensors created under torch.inference_mode() track no version counter: reading it raises)
    version = 0 if indices.is_inference() else indices._version
    key = (indices.data_ptr(), version, indices.shape[0], tuple(t.spatial_shape), t.batch_size)
    plan = cache.get(key)
    if plan is not None:
        return plan, feats, t
    recycled_key = next(iter(cache)) if len(cache) >= 2 else None
    try:
        if recycled_key is not None:
            plan = cache.pop(recycled_key)
            try:
                plan.rebuild(indices, t.batch_size, t.spatial_shape)
            except L.DpcgError:
                plan.close()
                raise
        else:
            plan = _UnetPlan(indices, t.batch_size, t.spatial_shape)
    except L.DpcgError as exc:
        if "sorted" not in str(exc) or _sorted_once:        # (sorting does not remove duplicate sites: one retry only)
            raise
        H, W = t.spatial_shape
        k = (indices[:, 0].long() * H + indices[:, 1].long()) * W + indices[:, 2].long()
        order = torch.argsort(k)
        return _plan_for(net, SparseBatch(feats[order], indices[order].contiguous(), t.spatial_shape, t.batch_size), True)
    cache[key] = plan
    return plan, feats, t


def hip_unet_forward(net, t: SparseBatch) -> SparseBatch:
    """`PreconditionerSparseUNet.forward` on the HIP path (call only when `hip_unet_applies`)."""
    from . import _lib as L
    layers = _unet_layers(net)
    with torch.cuda.device(t.features.device):
        plan, feats, t = _plan_for(net, t)
        n = len(layers)
        c = [net.enc1[0].in_channels, net.enc1[0].out_channels, net.down1[0].out_channels, net.down2[0].out_channels,
             net.down3[0].out_channels, net.bottleneck[0].out_channels]
        chan = (C.c_int32 * 6)(*c)
        dims = (C.c_int32 * (2 * n))(*[v for conv, _ in layers for v in (conv.weight.shape[3], conv.weight.shape[0])])
        ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p()       # noqa: E731
        keep = [conv.weight.detach().contiguous() for conv, _ in layers]
        w = (C.c_void_p * n)(*[ptr(x) for x in keep])
        b = (C.c_void_p * n)(*[ptr(conv.bias.detach() if conv.bias is not None else None) for conv, _ in layers])
        slopes = (C.c_float * n)(*[float(act.negative_slope) if act is not None else 0.0 for _, act in layers])
        out_feats = torch.empty((plan.sites, c[5]), dtype=torch.float32, device=feats.device)
        lower_val = torch.empty(plan.nnz_lower, dtype=torch.float64, device=feats.device)
        L.check(L.lib().dpcg_unet_forward(plan.handle, chan, dims, w, b, slopes, ptr(feats), int(feats.shape[1]), ptr(out_feats),
                                          ptr(lower_val), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    out = SparseBatch(out_feats, plan.out_indices, plan.out_shape, t.batch_size)
    out.lower_csr = (plan.lower_rowptr, plan.lower_col, lower_val)  # rows = batch * height, sample b at [b * H, (b + 1) * H)
    return out


def cached_plan(net, t: SparseBatch):
    """The plan the HIP path cached for the pattern of `t` (None before the first call)."""
    ptr = t.indices.contiguous().data_ptr()
    return next((p for p in net.__dict__.get("_hip_unet_plans", {}).values() if p.indices.data_ptr() == ptr), None)


def unet_forward_cost(net, t: SparseBatch) -> dict:
    """Flop and byte model of `PreconditionerSparseUNet.forward` on the HIP path for the pattern of `t` (whose plan must be
    cached: call the net once first), as `model.forward_cost` for `PreconditionerNet`.  Per layer: sites = output sites;
    flops = 2 * taps * C_in * C_out * sites (every tap of every output site is a C_in x C_out product on the matrix cores,
    absent neighbours included); bytes = the minimum the layer moves through HBM: its input features once
    (sites_in * C_in * 4), its output features (sites * C_out * 4; out_conv also writes the fp64 lower triangle of channel 0),
    its rulebook (taps * sites * 4) and, for up*, the skip it adds (sites * C_out * 4)."""
    layers = _unet_layers(net)
    plan = cached_plan(net, t)
    if plan is None or layers is None:
        raise ValueError("unet_forward_cost: run the net on this input first (HIP path, cached plan)")
    S = [lv["sites"] for lv in plan.levels]
    # (input level, output level) of each layer
    where = [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4),
             (4, 3), (3, 3), (3, 2), (2, 2), (2, 1), (1, 1), (1, 0), (0, 0), (0, 0)]
    out, total_f, total_b = [], 0, 0
    for name, (conv, _), (li, lo) in zip(LAYERS, layers, where):
        cin, cout = int(conv.weight.shape[3]), int(conv.weight.shape[0])
        taps = conv.kernel_size[0] * conv.kernel_size[1]
        sites = S[lo]
        flops = 2 * taps * cin * cout * sites
        byts = S[li] * cin * 4 + sites * cout * 4 + (taps * sites * 4 if taps > 1 else 0)
        if name.startswith("up"):
            byts += sites * cout * 4
        if name == "out_conv":
            byts += plan.nnz_lower * 8
        out.append({"layer": name, "kernel": list(conv.kernel_size), "c_in": cin, "c_out": cout, "sites": sites,
                    "flops": flops, "min_hbm_bytes": byts})
        total_f += flops
        total_b += byts
    return {"layers": out, "flops": total_f, "min_hbm_bytes": total_b}
