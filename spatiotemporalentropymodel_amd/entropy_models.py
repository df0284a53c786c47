"""EntropyModel / EntropyBottleneck / GaussianConditional with the reference's API
(compressai/entropy_models/entropy_models.py:68-604).

Device side (forward / likelihood / quantize / build_indexes, forward AND backward) = fused HIP
kernels.  Host side (`update()`: CDF tables once per model, `compress()` / `decompress()`: the
rANS coder) = numpy + libstem_rans.so, as north_star prescribes ("the rANS coder stays on host").
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import scipy.stats
import torch
import torch.nn as nn

from . import _lib
from . import functional as F
from .ops import LowerBound


# ----------------------------------------------------------------------------- host codec
def pmf_to_quantized_cdf(pmf, precision=16):
    """compressai._CXX.pmf_to_quantized_cdf (cpp_exts/ops/ops.cpp:24-81) -> torch.IntTensor"""
    p = np.ascontiguousarray(pmf.detach().cpu().numpy() if torch.is_tensor(pmf) else pmf, dtype=np.float32)
    cdf = np.empty(p.size + 1, np.uint32)
    lib = _lib.rans()
    if lib.stem_pmf_to_quantized_cdf(p.ctypes.data, p.size, int(precision), cdf.ctypes.data) != 0:
        raise ValueError(lib.stem_rans_last_error().decode())
    return torch.from_numpy(cdf.astype(np.int32))


class _Tables:
    """Dense int32 arrays of (cdf, cdf_length, offset) handed to libstem_rans.so without per-call conversion.  A tensor is COPIED:
    a numpy view of a host buffer would follow later writes into it and pin its storage (a table that numpy holds cannot be
    resized by update_registered_buffers)."""

    @staticmethod
    def _host(a):
        if torch.is_tensor(a):
            a = a.detach().to("cpu", torch.int32, copy=True).contiguous().numpy()
        return np.ascontiguousarray(a, dtype=np.int32)

    def __init__(self, cdf, sizes, offsets):
        self.cdf, self.sizes, self.offsets = self._host(cdf), self._host(sizes).reshape(-1), self._host(offsets).reshape(-1)
        assert self.cdf.ndim == 2 and self.cdf.shape[0] == self.sizes.size == self.offsets.size

    def args(self):
        return (self.cdf.ctypes.data, self.cdf.shape[0], self.cdf.shape[1], self.sizes.ctypes.data, self.offsets.ctypes.data)


def _i32(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32)


def _as_tables(cdfs, sizes, offsets):
    return cdfs if isinstance(cdfs, _Tables) else _Tables(np.asarray(cdfs, dtype=np.int32), sizes, offsets)


def _rans_err():
    return RuntimeError(_lib.rans().stem_rans_last_error().decode())


class RansEncoder:
    """compressai.ans.RansEncoder (cpp_exts/rans/rans_interface.cpp:193-204)."""

    def encode_with_indexes(self, symbols, indexes, cdfs, cdfs_sizes=None, offsets=None) -> bytes:
        t = _as_tables(cdfs, cdfs_sizes, offsets)
        sym, idx = _i32(symbols), _i32(indexes)
        if sym.size != idx.size:
            raise ValueError("symbols and indexes differ in length")
        cap = 8 * sym.size + 16
        out = np.empty(cap, np.uint8)
        n = _lib.rans().stem_rans_encode(sym.ctypes.data, idx.ctypes.data, sym.size, *t.args(), out.ctypes.data, cap)
        if n < 0:
            raise _rans_err()
        return out[:n].tobytes()


class BufferedRansEncoder:
    """compressai.ans.BufferedRansEncoder (rans_interface.cpp:99-191)."""

    def __init__(self):
        self._h = _lib.rans().stem_rans_encoder_create()
        self._destroy = _lib.rans().stem_rans_encoder_destroy      # bound now: module globals vanish at shutdown

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def encode_with_indexes(self, symbols, indexes, cdfs, cdfs_sizes=None, offsets=None) -> None:
        t = _as_tables(cdfs, cdfs_sizes, offsets)
        sym, idx = _i32(symbols), _i32(indexes)
        if _lib.rans().stem_rans_encoder_push(self._h, sym.ctypes.data, idx.ctypes.data, sym.size, *t.args()) != 0:
            raise _rans_err()

    def flush(self) -> bytes:
        lib = _lib.rans()
        cap = lib.stem_rans_encoder_pending_bytes(self._h)
        out = np.empty(cap, np.uint8)
        n = lib.stem_rans_encoder_flush(self._h, out.ctypes.data, cap)
        if n < 0:
            raise _rans_err()
        return out[:n].tobytes()


class RansDecoder:
    """compressai.ans.RansDecoder (rans_interface.cpp:206-350)."""

    def __init__(self):
        self._h = _lib.rans().stem_rans_decoder_create()
        self._destroy = _lib.rans().stem_rans_decoder_destroy

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def decode_with_indexes(self, encoded, indexes, cdfs, cdfs_sizes=None, offsets=None):
        return self.decode_with_indexes_np(encoded, indexes, cdfs, cdfs_sizes, offsets).tolist()

    def decode_with_indexes_np(self, encoded, indexes, cdfs, cdfs_sizes=None, offsets=None):
        t = _as_tables(cdfs, cdfs_sizes, offsets)
        buf = np.frombuffer(encoded, np.uint8)
        idx = _i32(indexes)
        out = np.empty(idx.size, np.int32)
        if _lib.rans().stem_rans_decode(buf.ctypes.data, buf.size, idx.ctypes.data, idx.size, *t.args(), out.ctypes.data) != 0:
            raise _rans_err()
        return out

    def set_stream(self, encoded) -> None:
        buf = np.frombuffer(encoded, np.uint8)
        if _lib.rans().stem_rans_decoder_set_stream(self._h, buf.ctypes.data, buf.size) != 0:
            raise _rans_err()

    def decode_stream(self, indexes, cdfs, cdfs_sizes=None, offsets=None):
        return self.decode_stream_np(indexes, cdfs, cdfs_sizes, offsets).tolist()

    def decode_stream_np(self, indexes, cdfs, cdfs_sizes=None, offsets=None):
        t = _as_tables(cdfs, cdfs_sizes, offsets)
        idx = _i32(indexes)
        out = np.empty(idx.size, np.int32)
        if _lib.rans().stem_rans_decoder_decode(self._h, idx.ctypes.data, idx.size, *t.args(), out.ctypes.data) != 0:
            raise _rans_err()
        return out


_ENTROPY_CODER = ["ans"]


def available_entropy_coders():
    """compressai/__init__.py:58-62 (the optional `rangecoder` pip package is not provided)."""
    return ["ans"]


def set_entropy_coder(entropy_coder):
    if entropy_coder not in available_entropy_coders():
        raise ValueError(f'Invalid entropy coder "{entropy_coder}", choose from({", ".join(available_entropy_coders())}).')
    _ENTROPY_CODER[0] = entropy_coder


def get_entropy_coder():
    return _ENTROPY_CODER[0]


class _EntropyCoder:
    def __init__(self, method):
        if not isinstance(method, str):
            raise ValueError(f'Invalid method type "{type(method)}"')
        if method not in available_entropy_coders():
            raise ValueError(f'Unknown entropy coder "{method}" (available: {", ".join(available_entropy_coders())})')
        self._encoder, self._decoder = RansEncoder(), RansDecoder()

    def encode_with_indexes(self, *args, **kwargs):
        return self._encoder.encode_with_indexes(*args, **kwargs)

    def decode_with_indexes(self, *args, **kwargs):
        return self._decoder.decode_with_indexes(*args, **kwargs)


# ----------------------------------------------------------------------------- autograd glue
class _EBFunction(torch.autograd.Function):
    """EntropyBottleneck.forward (entropy_models.py:424-452) as one kernel each way."""

    @staticmethod
    def forward(ctx, x, noise, medians, *tensors14):
        pack = F.eb_pack(list(tensors14))
        z_hat, lik = F.eb_forward(F.to_nhwc(x), pack, medians=medians, noise=noise)
        ctx.save_for_backward(z_hat, pack)
        return z_hat, lik

    @staticmethod
    def backward(ctx, dzhat, dlik):
        z_hat, pack = ctx.saved_tensors
        dlik = _dense(dlik)
        dzin = None if dzhat is None else _dense(dzhat)
        dz, dpack = F.eb_backward(z_hat, pack, dlik, dzhat_in=dzin)
        grads = [torch.empty((pack.shape[0], *s), device=pack.device) for s in _EB_SHAPES]
        F.eb_unpack_grads(dpack, grads)
        return (dz, None, None, *grads)


_EB_SHAPES = [(3, 1), (3, 1), (3, 1), (3, 3), (3, 1), (3, 1), (3, 3), (3, 1), (3, 1), (3, 3), (3, 1), (3, 1), (1, 3), (1, 1)]


class _EBFFunction(torch.autograd.Function):
    """_EBFunction for any `filters`: the general kernels (include/stem_eb_filters.h), one each way"""

    @staticmethod
    def forward(ctx, filters, x, noise, medians, *tensors):
        pack = F.ebf_pack(list(tensors), filters)
        z_hat, lik = F.ebf_forward(F.to_nhwc(x), pack, filters, medians=medians, noise=noise)
        ctx.filters, ctx.shapes = filters, [tuple(t.shape) for t in tensors]
        ctx.save_for_backward(z_hat, pack)
        return z_hat, lik

    @staticmethod
    def backward(ctx, dzhat, dlik):
        z_hat, pack = ctx.saved_tensors
        dlik = torch.zeros_like(z_hat) if dlik is None else _dense(dlik)
        dzin = None if dzhat is None else _dense(dzhat)
        dz, dpack = F.ebf_backward(z_hat, pack, dlik, ctx.filters, dzhat_in=dzin, want_dz=ctx.needs_input_grad[1],
                                   want_dpack=any(ctx.needs_input_grad[4:]))
        grads = [None] * len(ctx.shapes)
        if dpack is not None:
            grads = [torch.empty(s, device=pack.device) for s in ctx.shapes]
            F.ebf_unpack_grads(dpack, grads, ctx.filters)
        return (None, dz, None, None, *grads)


def _dense(t):
    t = F.to_nhwc(t)
    if F.nhwc_ld(t) != t.shape[1]:
        t = F.copy_channels(t, F.empty_nhwc(*t.shape, t.device))
    return t


class _GCFunction(torch.autograd.Function):
    """GaussianConditional.forward (entropy_models.py:588-596): quantize + likelihood + both LowerBounds."""

    @staticmethod
    def forward(ctx, y, scales, means, noise, scale_bound, lik_bound):
        y = _dense(y)
        B, Cc, H, W = y.shape
        # scales / means are usually the two halves of one EPM output (chunk(2,1)): equal pitch views
        sc, mu = F.to_nhwc(scales), F.to_nhwc(means)
        if F.nhwc_ld(sc) != F.nhwc_ld(mu):
            sc, mu = _dense(sc), _dense(mu)
        out, lik = F.gc_forward(y, sc, mu, noise=noise, scale_bound=scale_bound, lik_bound=lik_bound)
        ctx.bounds = (scale_bound, lik_bound)
        ctx.save_for_backward(out, sc, mu)
        return out, lik

    @staticmethod
    def backward(ctx, dout, dlik):
        out, sc, mu = ctx.saved_tensors
        B, Cc, H, W = out.shape
        dgp = F.empty_nhwc(B, 2 * Cc, H, W, out.device)
        dy = F.empty_nhwc(B, Cc, H, W, out.device) if ctx.needs_input_grad[0] else None
        F.gc_backward(out, sc, mu, _dense(dlik), dgp[:, :Cc], dgp[:, Cc:], dy=dy, scale_bound=ctx.bounds[0], lik_bound=ctx.bounds[1])
        if dy is not None and dout is not None:
            dy = F.add(dy, _dense(dout))
        return dy, dgp[:, :Cc], dgp[:, Cc:], None, None, None


class _GCScaleFunction(torch.autograd.Function):
    """GaussianConditional.forward with means=None (entropy_models.py:570-596): one launch each way, no mean tensor, the noise
    drawn inside the forward launch, the gradient arriving at `out` added inside the backward launch.  `noise`: what
    EntropyModel._noise_slot returned (training) or None (eval: round)."""

    @staticmethod
    def forward(ctx, y, scales, noise, scale_bound, lik_bound):
        y, sc = F.to_nhwc(y), F.to_nhwc(scales)
        out, lik = F.gc_scale_forward(y, sc, "round" if noise is None else "noise", **(noise or {}), scale_bound=scale_bound,
                                      lik_bound=lik_bound)
        ctx.bounds = (scale_bound, lik_bound)
        ctx.save_for_backward(out, sc)
        return out, lik

    @staticmethod
    def backward(ctx, dout, dlik):
        out, sc = ctx.saved_tensors
        B, Cc, H, W = out.shape
        dsc = F.empty_nhwc(B, Cc, H, W, out.device) if ctx.needs_input_grad[1] else None
        dy = F.empty_nhwc(B, Cc, H, W, out.device) if ctx.needs_input_grad[0] else None
        if dsc is not None or dy is not None:
            F.gc_scale_backward(out, sc, F.to_nhwc(dlik), dscales=dsc, dy=dy, dout=None if dout is None or dy is None else F.to_nhwc(dout),
                                scale_bound=ctx.bounds[0], lik_bound=ctx.bounds[1])
        return dy, dsc, None, None, None


# ----------------------------------------------------------------------------- modules
class EntropyModel(nn.Module):
    def __init__(self, likelihood_bound=1e-9, entropy_coder=None, entropy_coder_precision=16):
        super().__init__()
        if entropy_coder is None:
            entropy_coder = get_entropy_coder()
        self.entropy_coder = _EntropyCoder(entropy_coder)
        self.entropy_coder_precision = int(entropy_coder_precision)
        self.use_likelihood_bound = likelihood_bound > 0
        self._lik_bound = float(likelihood_bound)
        if self.use_likelihood_bound:
            self.likelihood_lower_bound = LowerBound(likelihood_bound)
        self.register_buffer("_offset", torch.IntTensor())
        self.register_buffer("_quantized_cdf", torch.IntTensor())
        self.register_buffer("_cdf_length", torch.IntTensor())
        # noise: counter-based Philox stream (seed, offset); `noise_source(shape, device)` overrides it (parity tests)
        self.noise_seed = 0x5713
        self._noise_offset = 0
        self.noise_source = None
        self.noise_epoch = None       # 1-element int64 device tensor: device-side draw count (captured hipGraphs)
        self._tables = None

    offset = property(lambda self: self._offset)
    quantized_cdf = property(lambda self: self._quantized_cdf)
    cdf_length = property(lambda self: self._cdf_length)

    def forward(self, *args):
        raise NotImplementedError()

    def _noise_like(self, x_nhwc):
        """U(-1/2, 1/2) with x's logical [B,C,H,W] shape, NHWC memory (replaces _get_noise_cached, :112-120)."""
        if self.noise_source is not None:
            n = self.noise_source(tuple(x_nhwc.shape), x_nhwc.device)
            return _dense(n.to(x_nhwc.device))
        out = F.uniform_noise_like(x_nhwc, self.noise_seed, self._noise_offset, epoch=self.noise_epoch)
        self._noise_offset += (x_nhwc.numel() + 3) // 4
        return out

    def _noise_slot(self, x_nhwc):
        """For kernels that draw their noise inline: either {"noise": tensor} (injected source) or the Philox coordinates
        {"seed", "offset", "epoch"} the next _noise_like(x) would have used -- and advance the stream past them."""
        if self.noise_source is not None:
            return {"noise": self._noise_like(x_nhwc)}
        slot = {"seed": self.noise_seed, "offset": self._noise_offset, "epoch": self.noise_epoch}
        self._noise_offset += (x_nhwc.numel() + 3) // 4
        return slot

    def quantize(self, inputs, mode, means=None):
        if mode not in ("noise", "dequantize", "symbols"):
            raise ValueError(f'Invalid quantization mode: "{mode}"')
        x = _dense(inputs.detach() if not inputs.requires_grad else inputs)
        if mode == "noise":
            if inputs.requires_grad:
                return inputs + self._noise_like(x)      # differentiable identity path (torch add; off the hot path)
            return F.add(x, self._noise_like(x))
        if means is not None:
            m = _dense(means.detach().expand_as(inputs).contiguous() if means.shape != inputs.shape else means.detach())
            x = F.sub(x, m)
        out = F.round_(x)
        if mode == "dequantize":
            return F.add(out, m) if means is not None else out
        return out.int()

    @staticmethod
    def dequantize(inputs, means=None):
        if means is not None:
            outputs = inputs.type_as(means)
            outputs += means
        else:
            outputs = inputs.float()
        return outputs

    def _pmf_to_cdf(self, pmf, tail_mass, pmf_length, max_length):
        """One quantised CDF row per distribution: its first pmf_length[i] masses followed by the tail mass, through
        pmf_to_quantized_cdf at the coder's precision, zero-padded to max_length + 2 entries (entropy_models.py:170-176)."""
        rows = torch.zeros((len(pmf_length), int(max_length) + 2), dtype=torch.int32)
        for row, masses, tail, n in zip(rows, pmf, tail_mass, pmf_length):
            q = pmf_to_quantized_cdf(torch.cat((masses[: int(n)], tail), dim=0), self.entropy_coder_precision)
            row[: q.numel()] = q
        return rows

    @staticmethod
    def _require_table(t, ndim, missing, what):
        # the reference's messages (entropy_models.py:178-199): callers and tests match on them
        if t.numel() == 0:
            raise ValueError(f"Uninitialized {missing}. Run update() first")
        if t.dim() != ndim:
            raise ValueError(f"Invalid {what} size {t.size()}")

    def _check_cdf_size(self):
        self._require_table(self._quantized_cdf, 2, "CDFs", "CDF")

    def _check_offsets_size(self):
        self._require_table(self._offset, 1, "offsets", "offsets")

    def _check_cdf_length(self):
        self._require_table(self._cdf_length, 1, "CDF lengths", "offsets")

    def host_tables(self) -> _Tables:
        """(cdf, length, offset) as dense host arrays, cached until the next update()/load_state_dict."""
        key = (self._quantized_cdf.data_ptr(), self._quantized_cdf._version, tuple(self._quantized_cdf.shape))
        if self._tables is None or self._tables[0] != key:
            self._check_cdf_size(), self._check_cdf_length(), self._check_offsets_size()
            self._tables = (key, _Tables(self._quantized_cdf, self._cdf_length, self._offset))
        return self._tables[1]

    def _scale_index_args(self):
        """(scale table, scale bound) of the in-kernel scale-to-index search; only a model with a scale table has them"""
        raise ValueError(f"{type(self).__name__} has no scale table: `scales` cannot be turned into indexes")

    @staticmethod
    def _elementwise_means(means, shape):
        """means of `shape` or one value per (batch, channel) -> NHWC-memory tensor of `shape` (None stays None)"""
        if means is None:
            return None
        means = means.detach()
        if tuple(means.shape) != tuple(shape):
            means = means.expand(shape).contiguous()
        return F.to_nhwc(means)

    def _compress(self, inputs, indexes=None, means=None, chan_means=None, scales=None, return_y_hat=False):
        """One stem_symbols_pack launch -> symbols (and, with indexes=None, the indexes: of `scales`, else the channel numbers) in
        the reference's flattening order, one copy to the host, the host coder once per batch element.  return_y_hat: -> (strings,
        stem_symbols_unpack of the symbols still on the device: the values `_decompress` of the strings gives, NHWC memory)."""
        x = F.to_nhwc(inputs.detach())
        m = self._elementwise_means(means, inputs.shape)
        t = self.host_tables()
        if indexes is None:
            table, bound = self._scale_index_args() if scales is not None else (None, 0.0)
            sc = F.to_nhwc(scales.detach()) if scales is not None else None
            si = F.symbols_pack(x, m, chan_means, sc, table, bound)
            sym, idx = si.cpu().numpy()
        else:
            si = F.symbols_pack(x, m, chan_means, want_indexes=False)
            sym = si[0].cpu().numpy()
            idx = indexes.int().cpu().contiguous().numpy()
        enc = RansEncoder()
        strings = [enc.encode_with_indexes(sym[i], idx[i], t) for i in range(sym.shape[0])]
        return (strings, F.symbols_unpack(si[0], m, chan_means)) if return_y_hat else strings

    def compress(self, inputs, indexes, means=None, scales=None, return_y_hat=False):
        """symbols = round(inputs - means) coded with the host rANS, one string per batch element (:201-233).  indexes=None with
        `scales` (not in the reference): the indexes build_indexes(scales) would give are computed by the launch that quantises.
        return_y_hat=True: -> (strings, what `decompress` of them returns), the second from the encoder's own symbols."""
        if len(inputs.size()) != 4:
            raise ValueError("Invalid `inputs` size. Expected a 4-D tensor.")
        if indexes is None:
            if scales is None or scales.size() != inputs.size():
                raise ValueError("`inputs` and `scales` should have the same size.")
        elif scales is not None:
            raise ValueError("`indexes` and `scales` are alternatives.")
        elif inputs.size() != indexes.size():
            raise ValueError("`inputs` and `indexes` should have the same size.")
        return self._compress(inputs, indexes, means=means, scales=scales, return_y_hat=return_y_hat)

    @staticmethod
    def _check_decompress_args(strings, indexes, means):
        # means may be per element or one value per (batch, channel) broadcast over the spatial dims
        problems = (
            (not isinstance(strings, (tuple, list)), "Invalid `strings` parameter type."),
            (isinstance(strings, (tuple, list)) and len(strings) != indexes.shape[0], "Invalid strings or indexes parameters"),
            (indexes.dim() != 4, "Invalid `indexes` size. Expected a 4-D tensor."),
        )
        for bad, msg in problems:
            if bad:
                raise ValueError(msg)
        if means is None:
            return
        if tuple(means.shape[:-2]) != tuple(indexes.shape[:-2]):
            raise ValueError("Invalid means or indexes parameters")
        per_channel = means.shape[2] == 1 and means.shape[3] == 1
        if tuple(means.shape) != tuple(indexes.shape) and not per_channel:
            raise ValueError("Invalid means parameters")

    def _decompress(self, strings, shape, indexes=None, means=None, chan_means=None, scales=None, device=None):
        """indexes (given, or by stem_symbols_pack without y: of `scales`, else the channel numbers) -> the host decoder once per
        batch element -> one copy up -> stem_symbols_unpack: NHWC-memory values of `shape`"""
        t = self.host_tables()
        shape = tuple(int(s) for s in shape)
        if indexes is None and scales is None:
            # the channel numbers depend on nothing the device holds: stated on the host, no launch and no copy
            idx = np.broadcast_to(np.arange(shape[1], dtype=np.int32)[None, :, None, None], shape)
        elif indexes is None:
            table, bound = self._scale_index_args()
            idx = F.symbols_pack(None, scales=F.to_nhwc(scales.detach()), table=table, scale_bound=bound)[1].cpu().numpy()
        else:
            idx = indexes.int().cpu().contiguous().numpy()
        dec = RansDecoder()
        vals = np.stack([dec.decode_with_indexes_np(s, idx[i], t).reshape(idx[i].shape) for i, s in enumerate(strings)])
        sym = torch.from_numpy(vals).to(device)
        return F.symbols_unpack(sym, self._elementwise_means(means, shape), chan_means)

    def decompress(self, strings, indexes, means=None, scales=None):
        """one string per batch element -> dequantised values (:235-279); argument errors are ValueError as upstream.
        indexes=None with `scales`: as in compress.  The result has NHWC memory."""
        if indexes is None:
            if scales is None:
                raise ValueError("Invalid `indexes` parameter: give indexes or scales.")
            like = scales
        elif scales is not None:
            raise ValueError("`indexes` and `scales` are alternatives.")
        else:
            like = indexes
        self._check_decompress_args(strings, like, means)
        return self._decompress(strings, like.shape, indexes, means=means, scales=scales, device=like.device)


class EntropyBottleneck(EntropyModel):
    def __init__(self, channels, *args, tail_mass=1e-9, init_scale=10, filters=(3, 3, 3, 3), **kwargs):
        # (3, 3, 3, 3) runs on the specialised kernels (stem_eb_*), any other tuple inside the caps on the general family
        # (stem_ebf_*, include/stem_eb_filters.h); refused before anything is allocated
        filters = tuple(int(f) for f in filters)
        if any(f < 1 for f in filters):
            raise ValueError(f"filters={filters}: every width must be at least 1")
        if not F.ebf_in_caps(filters):
            raise NotImplementedError(f"filters={filters}: the HIP bottleneck kernels take at most {F.EBF_MAX_FILTERS} filters "
                                      f"of width at most {F.EBF_MAX_WIDTH}")
        super().__init__(*args, **kwargs)
        self.channels = int(channels)
        self.filters = filters
        self.init_scale = float(init_scale)
        self.tail_mass = float(tail_mass)
        # Per-channel MLP 1 -> filters[0] -> ... -> filters[-1] -> 1 of the cumulative (entropy_models.py:303-340 upstream; 1 -> 3 -> 3
        # -> 3 -> 3 -> 1 by default).  Layer i maps widths[i] -> widths[i+1]; the initial values make softplus(matrix) a constant
        # 1 / (s * fan_out) with s = init_scale^(1 / layers), biases are U(-1/2, 1/2) (drawn layer by layer: the only RNG use), gate
        # factors 0.
        widths = (1, *self.filters, 1)
        n_layers = len(widths) - 1
        per_layer_scale = self.init_scale ** (1.0 / n_layers)
        C = self.channels
        for i, (fan_in, fan_out) in enumerate(zip(widths[:-1], widths[1:])):
            raw = float(np.log(np.expm1(1.0 / per_layer_scale / fan_out)))           # softplus^-1 of the target value
            self.register_parameter(f"_matrix{i:d}", nn.Parameter(torch.full((C, fan_out, fan_in), raw)))
            self.register_parameter(f"_bias{i:d}", nn.Parameter(torch.empty(C, fan_out, 1).uniform_(-0.5, 0.5)))
            if i < n_layers - 1:
                self.register_parameter(f"_factor{i:d}", nn.Parameter(torch.zeros(C, fan_out, 1)))
        # quantiles start at (-init_scale, 0, +init_scale); the aux loss pulls them to the tail_mass/2, 1/2, 1-tail_mass/2
        # points of the learned density, expressed as logits in `target`
        q0 = torch.tensor([-self.init_scale, 0.0, self.init_scale])
        self.quantiles = nn.Parameter(q0.expand(C, 1, 3).clone())
        tail_logit = float(np.log(2.0 / self.tail_mass - 1.0))
        self.register_buffer("target", torch.tensor([-tail_logit, 0.0, tail_logit]))

    @property
    def _specialised(self):
        """the default tuple: the specialised kernels (stem_eb_*) and the fused schedules; nothing is stored, so a module pickled
        before the general kernels existed behaves as it did"""
        return tuple(self.filters) == (3, 3, 3, 3)

    def _tensors14(self):
        """the 14 tensors of the specialised kernels' [C][58] pack; the fused schedules (engine, trainer, launch tape) know no other"""
        if not self._specialised:
            raise ValueError(f"EntropyBottleneck(filters={self.filters}): the fused schedule and its [C][58] pack exist for "
                             "filters=(3, 3, 3, 3) only; other filters run through the module's own forward / autograd")
        return [getattr(self, n) for n in F.EB_TENSORS]

    def _tensors(self):
        """the 3 L + 2 tensors in pack order (F.ebf_layout)"""
        return [getattr(self, n) for n in F.ebf_tensor_names(self.filters)]

    def _get_medians(self):
        return self.quantiles[:, :, 1:2]

    def _medians_vec(self):
        return self.quantiles.detach()[:, 0, 1].contiguous()

    # ---- host side -------------------------------------------------------------------------
    def _logits_cumulative_host(self, inputs):
        """entropy_models.py:388-407 on CPU tensors, used only by update() (once per model)."""
        logits = inputs
        for i in range(len(self.filters) + 1):
            matrix = getattr(self, f"_matrix{i:d}").detach().cpu()
            logits = torch.matmul(torch.nn.functional.softplus(matrix), logits)
            logits = logits + getattr(self, f"_bias{i:d}").detach().cpu()
            if i < len(self.filters):
                factor = getattr(self, f"_factor{i:d}").detach().cpu()
                logits = logits + torch.tanh(factor) * torch.tanh(logits)
        return logits

    def update(self, force=False):
        """Host side, once per model: the integer CDF tables of the learned density on the support the quantiles span
        (entropy_models.py:341-381; the arithmetic order is the reference's, the tables are compared entry by entry)."""
        if self._offset.numel() > 0 and not force:
            return False
        lo_q, med, hi_q = self.quantiles.detach().cpu()[:, 0, :].unbind(dim=1)
        left = torch.clamp(torch.ceil(med - lo_q).int(), min=0)           # integer steps covered below / above the median
        right = torch.clamp(torch.ceil(hi_q - med).int(), min=0)
        length = right + left + 1
        longest = length.max()
        grid = torch.arange(longest)[None, :] + (med - left)[:, None, None]      # [C, 1, longest] sample positions
        lower, upper = self._logits_cumulative_host(grid - 0.5), self._logits_cumulative_host(grid + 0.5)
        flip = -torch.sign(lower + upper)                  # evaluate the difference of sigmoids on the numerically safe side
        mass = torch.abs(torch.sigmoid(flip * upper) - torch.sigmoid(flip * lower))[:, 0, :]
        tails = torch.sigmoid(lower[:, 0, :1]) + torch.sigmoid(-upper[:, 0, -1:])
        dev = self.quantiles.device
        self._quantized_cdf = self._pmf_to_cdf(mass, tails, length, longest).to(dev)
        self._offset = (-left).to(dev)
        self._cdf_length = (length + 2).to(dev)
        self._tables = None
        return True

    # ---- device side -----------------------------------------------------------------------
    def _noise_like(self, x_nhwc):
        """The reference draws bottleneck noise in [C,1,H*W*B] order (entropy_models.py:426-434); an injected
        noise_source is asked for that shape and re-laid out so parity tests can feed the same numbers."""
        if self.noise_source is not None:
            B, Cc, H, W = x_nhwc.shape
            n = self.noise_source((Cc, 1, H * W * B), x_nhwc.device)
            n = n.reshape(Cc, H, W, B).permute(3, 0, 1, 2)
            return _dense(n.to(x_nhwc.device).contiguous())
        return super()._noise_like(x_nhwc)

    def loss(self):
        """Auxiliary loss (entropy_models.py:383-386); gradient flows to `quantiles` only."""
        if not self._specialised:
            return _EBFAuxFunction.apply(self.filters, self.quantiles, self.target, *self._tensors())
        return _EBAuxFunction.apply(self.quantiles, self.target, *self._tensors14())

    def forward(self, x):
        xin = F.to_nhwc(x)
        if self.training:
            noise, med = self._noise_like(xin), None
        else:
            noise, med = None, self._medians_vec()
        if not self._specialised:
            return _EBFFunction.apply(self.filters, x, noise, med, *self._tensors())
        return _EBFunction.apply(x, noise, med, *self._tensors14())

    @staticmethod
    def _build_indexes(size):
        N, Cc, H, W = size
        indexes = torch.arange(Cc).view(1, -1, 1, 1)
        return indexes.int().repeat(N, 1, H, W)

    def compress(self, x, return_y_hat=False):
        """the medians go in as one value per channel and the indexes are the channel numbers (`_build_indexes`), both inside the launch"""
        if len(x.size()) != 4:
            raise ValueError("Invalid `inputs` size. Expected a 4-D tensor.")
        return self._compress(x, chan_means=self._medians_vec(), return_y_hat=return_y_hat)

    def decompress(self, strings, size):
        if not isinstance(strings, (tuple, list)):
            raise ValueError("Invalid `strings` parameter type.")
        output_size = (len(strings), self._quantized_cdf.size(0), size[0], size[1])
        return self._decompress(strings, output_size, chan_means=self._medians_vec(), device=self._quantized_cdf.device)


class _EBAuxFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, quantiles, target, *tensors14):
        pack = F.eb_pack(list(tensors14))
        loss, dq = F.eb_aux_loss(quantiles, pack, target)
        ctx.save_for_backward(dq)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dq,) = ctx.saved_tensors
        return (dq * g, None) + (None,) * 14


class _EBFAuxFunction(torch.autograd.Function):
    """_EBAuxFunction for any `filters`: the general kernel (stem_ebf_aux_loss_grad)"""

    @staticmethod
    def forward(ctx, filters, quantiles, target, *tensors):
        pack = F.ebf_pack(list(tensors), filters)
        q = quantiles.detach().contiguous()
        dq = torch.empty_like(q)
        loss = F.ebf_aux_loss_grad(q, pack, target, filters, dq)
        ctx.save_for_backward(dq)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dq,) = ctx.saved_tensors
        return (None, dq * g, None) + (None,) * (len(ctx.needs_input_grad) - 3)


class GaussianConditional(EntropyModel):
    def __init__(self, scale_table, *args, scale_bound=0.11, tail_mass=1e-9, **kwargs):
        super().__init__(*args, **kwargs)
        if not isinstance(scale_table, (type(None), list, tuple)):
            raise ValueError(f'Invalid type for scale_table "{type(scale_table)}"')
        if isinstance(scale_table, (list, tuple)) and len(scale_table) < 1:
            raise ValueError(f'Invalid scale_table length "{len(scale_table)}"')
        if scale_table and (scale_table != sorted(scale_table) or any(s <= 0 for s in scale_table)):
            raise ValueError(f'Invalid scale_table "({scale_table})"')
        self.tail_mass = float(tail_mass)
        if scale_bound is None and scale_table:
            scale_bound = float(scale_table[0])
            self.lower_bound_scale = LowerBound(scale_bound)
            register_bound = None
        elif scale_bound is not None and scale_bound > 0:
            self.lower_bound_scale = LowerBound(scale_bound)
            register_bound = torch.Tensor([float(scale_bound)])
        else:
            raise ValueError("Invalid parameters")
        self._scale_bound = float(scale_bound)
        self.register_buffer("scale_table", self._prepare_scale_table(scale_table) if scale_table else torch.Tensor())
        self.register_buffer("scale_bound", register_bound)

    @staticmethod
    def _prepare_scale_table(scale_table):
        return torch.Tensor(tuple(float(s) for s in scale_table))

    @staticmethod
    def _standardized_cumulative(inputs):
        return float(0.5) * torch.erfc(float(-(2 ** -0.5)) * inputs)

    @staticmethod
    def _standardized_quantile(quantile):
        return scipy.stats.norm.ppf(quantile)

    def update_scale_table(self, scale_table, force=False):
        """Install a scale table and rebuild the CDF tables; a no-op (False) when tables exist and force is not set
        (entropy_models.py:535-541)."""
        if self._offset.numel() > 0 and not force:
            return False
        self.scale_table = self._prepare_scale_table(scale_table).to(self.scale_table.device)
        self.update()
        return True

    def update(self):
        """Host side, once per model (entropy_models.py:543-568): per table scale the zero-mean Gaussian's mass on the integers
        within the tail_mass quantile, symmetric about 0, as integer CDF rows."""
        sigma = self.scale_table.detach().cpu()
        reach = torch.ceil(sigma * (-self._standardized_quantile(self.tail_mass / 2))).int()      # half width of the support
        length = 2 * reach + 1
        longest = torch.max(length).item()
        dist = torch.abs(torch.arange(longest).int() - reach[:, None]).float()                    # |k - centre|
        s = sigma.unsqueeze(1).float()
        upper = self._standardized_cumulative((0.5 - dist) / s)
        lower = self._standardized_cumulative((-0.5 - dist) / s)
        dev = self.scale_table.device
        self._quantized_cdf = self._pmf_to_cdf(upper - lower, 2 * lower[:, :1], length, longest).to(dev)
        self._offset = (-reach).to(dev)
        self._cdf_length = (length + 2).to(dev)
        self._tables = None

    def forward(self, inputs, scales, means=None):
        if means is None:
            # entropy_models.py:570-596 with means=None: quantize(inputs) without an offset, likelihood of the values themselves.  The
            # zero-mean kernels compute what the mean kernels compute from a tensor of zeros, value for value and gradient bit for
            # bit, except that an eval-mode round(-0.3) stays the reference's -0.0 (round(x - 0) + 0 made it +0.0).  The noise is
            # drawn in the launch, from the stream coordinates _noise_like would have used.
            noise = self._noise_slot(F.to_nhwc(inputs.detach())) if self.training else None
            return _GCScaleFunction.apply(inputs, scales, noise, self._scale_bound, self._lik_bound if self.use_likelihood_bound else 0.0)
        noise = self._noise_like(_dense(inputs.detach())) if self.training else None
        return _GCFunction.apply(inputs, scales, means, noise, self._scale_bound, self._lik_bound if self.use_likelihood_bound else 0.0)

    def build_indexes(self, scales):
        return F.build_indexes(F.to_nhwc(scales.detach()), self.scale_table, self._scale_bound)

    def _scale_index_args(self):
        return self.scale_table, self._scale_bound
