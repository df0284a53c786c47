"""StemEngine: the whole-model forward / backward schedule of a STEM entropy model as a flat sequence
of C-ABI kernel launches (no per-layer autograd nodes, no concatenations, no activation passes).

Mirrors, for all five model variants, the dataflow of
  compressai/models/spatiotemporalpriors.py:70-83, 176-194, 292-311, 561-585, 845-868 (forward)
and what torch autograd derives from it for `EMLoss` (utils.py:18-27) with y_cur / y_conditioned
detached (stem/trainSTEM.py:208).

Memory plan (NHWC fp32): `he_in` = [y_cur | y_cond] and `epm_in` = [tp | hp | ctx]
are single buffers whose channel slices are written in place by their producers; the EPM output
`gp` is read as (scales | means) slices by the Gaussian kernel.  LeakyReLU is fused into the
producing convolution (forward) and into the consuming dgrad's epilogue (backward).
"""
from __future__ import annotations

import collections

import torch

from . import _lib
from . import config as _config
from . import functional as F
from . import layers as _layers

class _Switch:
    """A StemEngine switch backed by a field of config.StemRuntimeConfig, read when it is LOOKED UP: `config.override(...)` takes
    effect at once, a changed `STEM_*` variable when the next engine is built (StemEngine.__init__ parses the environment again;
    a look-up itself reads the parsed object -- 0.1 us instead of 15 -- because the schedule asks ~50 times per step).  The route
    switches are looked up when an engine is built, the scheduling ones at every step.  A plain value assigned on the class or on
    an instance (`StemEngine.use_fx3 = False`, tests' monkeypatch) wins."""

    def __init__(self, field):
        self.field = field

    def __get__(self, obj, owner=None):
        return getattr(_config._RUNTIME or _config.runtime(), self.field)


class _Act:
    """One activation of the schedule: the fp32 NHWC tensor `x`, its fp16 planes `p` (None until an epilogue wrote them or planes()
    split them) and `rec`, the scale record the producer of `x` left (None: a split measures x itself)."""
    __slots__ = ("x", "p", "rec")

    def __init__(self, x, p=None, rec=None):
        self.x, self.p, self.rec = x, p, rec

    def planes(self, record=True):
        """the planes, split on the current stream at the first request"""
        if self.p is None:
            self.p = F.F16Planes.split(self.x, src_q=self.rec.data_ptr() if record and self.rec is not None else None)
        return self.p

    def channels(self, c0, c1):
        """a channel range of both members (planes views are 32-channel aligned)"""
        return _Act(self.x[:, c0:c1], None if self.p is None else self.p.channels(c0, c1))


#: one face (forward / input gradient) of a layer: kind "gen" (general fp16 kernel), "phases" (the same kernel over the four sub-pixel
#: phases of a transposed face) or "f32" (igemm.hip), and the (outputs, contraction channels, flip, taps) of its packed weight image
_Face = collections.namedtuple("_Face", "kind N C flip taps")


class _Layer:
    """One convolution of the schedule: parameters, persistent packed-weight buffers and wgrad slabs."""

    def __init__(self, mod, kind, eng):
        self.mod, self.kind, self.eng = mod, kind, eng      # kind: "conv" | "deconv"
        self.R = mod.kernel_size
        self.stride, self.pad = mod.stride, mod.padding
        self.opad = getattr(mod, "output_padding", 0)
        self.K, self.C = mod.out_channels, mod.in_channels
        self.masked = getattr(mod, "_masked", 0)
        self.wp_fwd = self.wp_dgrad = None
        self.need_dgrad = True
        # forward / input-gradient on the fp16 matrix cores (csrc/conv_f16x3.hip, general variant): stride-1 convolutions whose
        # contraction channels are multiples of 32; decided once by the engine (StemEngine._select_fx3)
        self.fx3 = False
        self.wg3 = False
        self.taps = 0             # masked convolution on the fp16 kernel: the number of live taps (a prefix of the row-major order)
        # fx3s: the STRIDED-CONVOLUTION face of a stride-2 layer on the general fp16 kernel -- the forward of a strided Conv2d
        # (HE.2 / HE.4), the input gradient of a ConvTranspose2d (HD.0 / HD.2: a strided convolution of dy with the stored weight
        # [C][K][R][S] read as a Conv2d weight with C outputs); the transposed face stays on igemm.hip's sub-pixel phases
        self.fx3s = False
        # fx3t: ... and the TRANSPOSED face too (forward of a ConvTranspose2d, input gradient of a strided Conv2d) as one launch of the
        # same kernel over its four sub-pixel phases (F.tconv2d_f16x3), and the layer's weight gradient on the per-tap fp16 kernel
        # with a strided gather (F.conv2d_wgrad_f16x3_strided): no fp32-MFMA launch is left in the layer
        self.fx3t = False
        self.wp6_fwd = self.wp6_dgrad = None
        self._slabs = {}
        self.pending = None       # (dwp, splits) of the last wgrad, consumed by StemEngine.unpack_all
        self.lane = 0             # which weight-gradient stream this layer's wgrad / unpack runs on (StemEngine.side_stream)
        self.tail_event = None    # the event behind this layer's images when an ordered optimiser tail packed them off the compute stream
        self.tail_group = 0       # ... and the group of that tail (StemEngine.tail_plan)

    def fx3_eligible(self):
        return self.kind == "conv" and not self.masked and _layers.f16x3_same_shape(self.stride, self.R, self.pad, self.C, self.K)

    def fx3_masked_eligible(self):
        """the context model's masked convolution, forward only (its input is data + noise: no input gradient): the general
        kernel runs over the live taps alone -- 12 of 25 for the 5x5 type-A mask (layers.py:21-47)"""
        return (self.kind == "conv" and bool(self.masked) and not self.need_dgrad
                and _layers.f16x3_same_shape(self.stride, self.R, self.pad, self.C, self.K, k_multiple=4))

    def fx3s_eligible(self):
        n_out, n_red = (self.K, self.C) if self.kind == "conv" else (self.C, self.K)       # outputs / contraction channels of that face
        return (self.stride == 2 and not self.masked and n_red % 32 == 0 and n_out % 4 == 0 and self.R * self.R <= 25
                and (self.kind == "conv" or self.need_dgrad))

    def fx3t_eligible(self):
        """both faces and the weight gradient on the fp16 kernels: 5x5 / 3x3, stride 2, padding R // 2, the ConvTranspose2d with
        output_padding 1 (fine grid = twice the coarse grid), channel counts in whole 32-channel slabs"""
        return (self.fx3s and self.R % 2 == 1 and self.R >= 3 and self.pad == self.R // 2 and self.C % 32 == 0 and self.K % 32 == 0
                and (self.kind == "conv" or self.opad == 1))

    def wg3_eligible(self):
        """weight gradient on csrc/wgrad_f16x3.hip: stride-1 convolutions (all taps are produced, as autograd does for the
        masked context convolution too)"""
        return self.kind == "conv" and _layers.f16x3_same_shape(self.stride, self.R, self.pad, self.C, self.K)

    def set_faces(self):
        """The ONE description of which kernel serves the layer's two faces, derived from the route flags when the engine has
        chosen them (StemEngine._select_fx3): packing, allocation and the three compute methods below all read it."""
        K, C, conv = self.K, self.C, self.kind == "conv"
        fwd = dgrad = _Face("f32", K, C, 0, 0)
        if self.fx3:              # the input gradient of a stride-1 convolution is a convolution with the mirrored, transposed weight
            fwd, dgrad = _Face("gen", K, C, 0, self.taps), _Face("gen", C, K, 1, 0)
        elif self.fx3s:
            # strided face: the torch weight read as a Conv2d weight [outputs][contraction]; transposed face: read as w[c][n] (flip = 2)
            if conv:
                fwd, dgrad = _Face("gen", K, C, 0, 0), (_Face("phases", C, K, 2, 0) if self.fx3t else dgrad)
            else:
                fwd, dgrad = (_Face("phases", K, C, 2, 0) if self.fx3t else fwd), _Face("gen", C, K, 0, 0)
        self.faces = (fwd, dgrad if self.need_dgrad else None)

    def alloc_packs(self, device):
        """exactly the packed weight copies the two faces read: fp32 (wp_*) for igemm.hip, an fp16 image (wp6_*) otherwise"""
        bufs = []
        for face in self.faces:
            if face is None:
                bufs += [None, None]
            elif face.kind == "f32":
                bufs += [torch.empty(self.K * self.C * self.R * self.R, device=device, dtype=torch.float32), None]
            else:                 # (zeros: the pair pack never writes the padding rows of a 128-row tile)
                bufs += [None, torch.zeros(F.f16x2_gen_weight_bytes(face.N, face.C, self.R, self.R), device=device, dtype=torch.uint8)]
        self.wp_fwd, self.wp6_fwd, self.wp_dgrad, self.wp6_dgrad = bufs
        if self.fx3s and self.wp_fwd is None:
            self.wp_fwd = torch.empty(0, device=device)              # never read: a stride-2 layer without an fp32 forward copy

    def role_descs(self, role):
        """(fp32 descriptors, fp16 descriptors) of this layer's packed copies for role 0 (forward) / 1 (input gradient)"""
        face = self.faces[role]
        if face is None:
            return [], []
        if face.kind == "f32":
            return [self._desc32(role)], []
        wp = self.wp6_dgrad if role else self.wp6_fwd
        return [], [_lib.F16PackDesc(self.mod.weight.data_ptr(), wp.data_ptr(), face.N, face.C, self.R, self.R, face.flip, face.taps)]

    def pair_desc(self):
        """both fp16 images of this layer as ONE descriptor of the pair pack (F.pack_weights_f16x2_pair_multi), or None when the
        layer keeps an fp32 copy of a role"""
        a, b = self.role_descs(0), self.role_descs(1)
        if a[0] or b[0] or not a[1]:
            return None
        w = self.mod.weight
        A, Bd = int(w.shape[0]), int(w.shape[1])
        roles = []
        for d in (a[1][0], b[1][0] if b[1] else None):
            if d is None:
                roles += [None, 0, 0]
                continue
            rows_b = int(d.flip != 0)
            assert (d.N, d.C) == ((Bd, A) if rows_b else (A, Bd)), "pair pack: a role image must be a transpose of the tensor itself"
            roles += [d.wp, rows_b | (int(d.flip) << 1), int(d.taps)]
        return _lib.F16PairDesc(w.data_ptr(), A, Bd, self.R, self.R, roles[0], roles[1], roles[2], roles[3], roles[4], roles[5], None, 0, 0)

    def _desc32(self, role):
        w = self.mod.weight
        conv = self.kind == "conv"
        if role == 0:
            return _lib.PackDesc(w.data_ptr(), self.wp_fwd.data_ptr(), self.K, self.C, self.R, self.R,
                                 F.PACK_CONV_FWD if conv else F.PACK_DECONV_FWD, self.masked)
        return _lib.PackDesc(w.data_ptr(), self.wp_dgrad.data_ptr(), self.K, self.C, self.R, self.R,
                             F.PACK_CONV_DGRAD if conv else F.PACK_DECONV_DGRAD, (1 | (self.masked & 4)) if self.masked else 0)

    # ---- the three operations of the schedule; each picks its kernel from `faces` / the route flags and nothing else -----------------
    def forward(self, a, act=F.ACT_NONE, out=None, planes=False):
        """a: _Act -> _Act of the (activated) output; `out` may be a channel slice of a wider NHWC buffer; planes: the fp16
        kernels write the output's planes next to the fp32 copy (the fp32 kernels cannot: the consumer splits)"""
        self.eng.ensure_packed()
        if self.tail_event is not None:
            self.eng._wait_tail(self)
        face, m = self.faces[0], self.mod
        epi = F.GEN_EPI_LRELU if act == F.ACT_LRELU else F.GEN_EPI_BIAS
        if face.kind == "gen":
            return _Act(*F.conv2d_f16x3_gen(a.planes(), self.wp6_fwd, m.bias, self.K, self.R, self.R, self.stride, self.pad,
                                            epi=epi, out=out, want_planes=planes, taps=self.taps))
        if face.kind == "phases":         # a ConvTranspose2d over its four sub-pixel phases, one launch
            return _Act(*F.tconv2d_f16x3(a.planes(), self.wp6_fwd, m.bias, self.K, self.R, epi=epi, out=out, want_planes=planes))
        self.eng._wait_fwd32_packs()
        if self.kind == "conv":
            if self.masked and not self.masked & 4:
                act |= F.CONV_MASKED_A            # the masked taps (type A) are zeros: skip them
            return _Act(F.conv2d_fwd(a.x, self.wp_fwd, m.bias, self.K, self.R, self.R, self.stride, self.pad, act, out=out))
        return _Act(F.deconv2d_fwd(a.x, self.wp_fwd, m.bias, self.K, self.R, self.R, self.stride, self.pad, self.opad, act, out=out))

    def fwd(self, x, act=F.ACT_NONE, out=None):
        """fp32 tensor in, fp32 tensor out: callers outside the training schedule (codec.py)"""
        return self.forward(_Act(x), act, out=out).x

    def input_grad(self, dy, xact=None, planes=False, x_shape=None):
        """dy: _Act -> _Act of the gradient of the layer's input; xact: the activated input (its leaky-ReLU derivative is folded
        in); x_shape: the input's shape where there is no xact (only the fp32 kernels ask)"""
        if self.tail_event is not None:
            self.eng._wait_tail(self)
        face = self.faces[1]
        epi = F.GEN_EPI_DACT if xact is not None else F.GEN_EPI_BIAS
        if face.kind == "gen":            # stride 1: the mirrored weight; a ConvTranspose2d: the strided convolution of dy with the stored weight
            return _Act(*F.conv2d_f16x3_gen(dy.planes(), self.wp6_dgrad, None, self.C, self.R, self.R, self.stride, self.pad,
                                            epi=epi, z=xact, want_planes=planes))
        if face.kind == "phases":         # a strided Conv2d: the transposed face
            return _Act(*F.tconv2d_f16x3(dy.planes(), self.wp6_dgrad, None, self.C, self.R, epi=epi, z=xact, want_planes=planes,
                                         fine_hw=tuple(xact.shape[2:]) if xact is not None else None))
        x_shape = xact.shape if xact is not None else x_shape
        if self.kind == "conv":
            return _Act(F.conv2d_dgrad(dy.x, self.wp_dgrad, x_shape, self.K, self.R, self.R, self.stride, self.pad, xact=xact))
        return _Act(F.deconv2d_dgrad(dy.x, self.wp_dgrad, x_shape, self.K, self.R, self.R, self.stride, self.pad, self.opad, xact=xact))

    def reads_dy_planes(self, x):
        """whether the gradient of this layer's output is wanted as planes too: the input gradient reads them, or the weight gradient
        of a chain's first layer does next to the planes of its input `x`"""
        return self.faces[1].kind != "f32" if self.faces[1] is not None else (self.wg3 and x.p is not None)

    def weight_grad(self, x, dy):
        """Weight + bias gradient from the layer's input `x` and output gradient `dy` (_Act): packed slabs now, StemEngine.unpack_all()
        / _group_ready turn every layer's slabs into .grad tensors with one launch.  A stride-1 layer with `wg3` takes the fp16 kernel
        when both operands have planes already -- they do whenever its two faces run on the fp16 kernels -- and a chain's first layer
        (no input gradient) when one has: the other is split here, on the compute stream, measuring its own maximum.  Runs on the
        engine's weight-gradient stream (nothing on the dgrad chain consumes it), ordered after everything the compute stream has
        queued so far."""
        at_hand = (x.p is not None) + (dy.p is not None)
        if self.fx3t:                     # fine-grid operand first: a Conv2d's input, a ConvTranspose2d's output gradient
            fn, args = self._wgrad_t, ((x.planes(), dy.planes()) if self.kind == "conv" else (dy.planes(), x.planes())) + (dy.x,)
        elif self.wg3 and at_hand >= (2 if self.need_dgrad else 1):
            fn, args = self._wgrad3, (x.planes(record=False), dy.planes(record=False), dy.x)
        else:
            fn, args = self._wgrad, (x.x, dy.x)
        side = self.eng.side_stream(dy.x.device, self.lane)
        if side is None:
            return fn(*args)
        F.stream_wait(side, F.cur_stream(dy.x.device))
        with F.on_stream(side):
            fn(*args)
        for t in args:
            (t.data if isinstance(t, F.F16Planes) else t).record_stream(side)

    def _wgrad_t(self, fine_p, coarse_p, dy):
        """a stride-2 layer from planes: `fine_p` the fine-grid operand, `coarse_p` the coarse-grid one; dy: the fp32 output
        gradient (bias column sums of the transposed layer)"""
        conv = self.kind == "conv"
        Kk = self.K if conv else self.C                  # rows of the slabs = channels of the coarse operand
        key = ("fp16t",) + tuple(fine_p.shape)
        if key not in self._slabs:
            splits, elems = F.wgrad_f16x3_strided_plan(fine_p.shape, Kk, self.R, self.R, self.stride, self.pad)
            self._slabs[key] = (torch.empty(elems, device=dy.device, dtype=torch.float32), splits,
                                torch.empty(splits * Kk, device=dy.device, dtype=torch.float32))
        dwp, splits, bpart = self._slabs[key]
        gb = _grad_of(self.mod.bias) if self.mod.bias is not None else None
        F.conv2d_wgrad_f16x3_strided(fine_p, coarse_p, Kk, self.R, self.R, self.stride, self.pad, dwp, splits,
                                     bias_part=bpart if (conv and gb is not None) else None)
        self.pending_bias = None
        if gb is not None and conv:                      # column sums of dy came out of the kernel: second stage
            self.pending_bias = _lib.BiasFinalDesc(bpart.data_ptr(), gb.data_ptr(), self.K, splits, int(self.eng.accumulate_grads), 0)
        elif gb is not None:                             # the transposed layer's bias sees the FINE tensor: its own column sums
            F.bias_grad(dy, gb, accumulate=self.eng.accumulate_grads)
        self.pending = (dwp, splits)

    def _wgrad3(self, xp, dyp, dy):
        key = ("fp16",) + tuple(xp.shape)
        if key not in self._slabs:
            splits, elems = F.wgrad_f16x3_plan(xp.shape, self.K, self.R, self.R, self.pad)
            self._slabs[key] = (torch.empty(elems, device=dy.device, dtype=torch.float32), splits,
                                torch.empty(splits * self.K, device=dy.device, dtype=torch.float32))
        dwp, splits, bpart = self._slabs[key]
        gb = _grad_of(self.mod.bias) if self.mod.bias is not None else None
        self.pending_bias = F.conv2d_wgrad_f16x3(xp, dyp, self.K, self.R, self.R, self.pad, dwp, splits, db=gb, bias_part=bpart,
                                                 accumulate_db=self.eng.accumulate_grads, defer_bias=True)
        self.pending = (dwp, splits)

    def _wgrad(self, x, dy):
        m = self.mod
        gb = _grad_of(m.bias)
        deconv = self.kind == "deconv"
        key = tuple(x.shape)
        key = key + (F.nhwc_ld(x), F.nhwc_ld(dy))          # the gather table bakes in the pitch of the gathered tensor
        fresh = key not in self._slabs
        if fresh:
            splits, elems = F.wgrad_plan(x.shape, self.K, self.R, self.R, self.stride, self.pad, deconv=deconv)
            self._slabs[key] = (torch.empty(elems, device=x.device, dtype=torch.float32), splits)
        dwp, splits = self._slabs[key]
        defer = gb is not None
        if deconv:
            _, b = F.deconv2d_wgrad(x, dy, self.K, self.R, self.R, self.stride, self.pad, self.opad, db_out=gb, dwp=dwp, unpack=False,
                                    table_valid=not fresh, accumulate_db=self.eng.accumulate_grads, defer_bias=defer)
        else:
            _, b = F.conv2d_wgrad(x, dy, self.K, self.R, self.R, self.stride, self.pad, db_out=gb, dwp=dwp, unpack=False,
                                  table_valid=not fresh, accumulate_db=self.eng.accumulate_grads, defer_bias=defer)
        self.pending_bias = b if defer else None          # the second stage joins the module group's launch (_group_ready_on_stream)
        self.pending = (dwp, splits)

    def unpack_desc(self):
        dwp, splits = self.pending
        self.pending = None
        return _lib.UnpackDesc(dwp.data_ptr(), _grad_of(self.mod.weight).data_ptr(), self.K, self.C, self.R, self.R, splits,
                               (F.UNPACK_DECONV if self.kind == "deconv" else 0) | (F.UNPACK_ACCUMULATE if self.eng.accumulate_grads else 0))


def _attach_block_maxima(d, numel, maxima, flat, ch=None):
    """point one fp16 pack descriptor (single or pair; numel: the elements of its weight) at the optimiser's chunk maxima that cover
    the weight inside the flat parameter buffer `flat`.  -> False, the descriptor untouched, when the weight lies outside the buffer"""
    off = (d.w - flat.data_ptr()) // 4
    if (d.w - flat.data_ptr()) % 4 or off < 0 or off + numel > flat.numel():
        return False
    ch = ch or F.adam_chunk()
    d.bmax, d.b0 = maxima.data_ptr(), off // ch
    d.nb = (off + numel - 1) // ch - d.b0 + 1
    return True


def tail_chunk_ranges(tensors, numel, ch, ngroups):
    """tensors: (offset, elements, group) of every tensor of a flat buffer of `numel` elements -> per group the list of chunk ranges
    [c0, c1) (chunks of `ch` elements) it owns.  A chunk belongs to the earliest group of any tensor it touches (one that touches
    none -- padding -- to group 0); the ranges of all groups together cover every chunk exactly once."""
    nch = (numel + ch - 1) // ch
    cgroup = [ngroups] * nch
    for off, n, gi in tensors:
        for c in range(off // ch, (off + max(n, 1) - 1) // ch + 1):
            cgroup[c] = min(cgroup[c], gi)
    out = [[] for _ in range(ngroups)]
    c = 0
    while c < nch:
        gi, c1 = cgroup[c], c
        while c1 < nch and cgroup[c1] == gi:
            c1 += 1
        out[0 if gi == ngroups else gi].append((c, c1))
        c = c1
    return out


def _grad_of(p):
    if p.grad is None:
        owner = getattr(p, "_flat_grad_view", None)
        # a fresh slot starts at zero: every producer below ADDS into it (autograd's `.grad +=`)
        p.grad = owner if owner is not None else torch.zeros_like(p, memory_format=torch.contiguous_format)
    return p.grad


class StemEngine:
    def __init__(self, model, has_tpm: bool, has_spm: bool, residual: bool):
        _config.runtime()                   # parse the environment now if a STEM_* variable changed (the switches read the parsed object)
        self.m = model
        eb_filters = tuple(model.entropy_bottleneck.filters)
        if eb_filters != (3, 3, 3, 3):
            # the schedule, the fused trainer and the launch tape call the specialised stem_eb_*_train* kernels on the [C][58] pack
            raise ValueError(f"StemEngine: the fused schedule is built for an EntropyBottleneck with filters=(3, 3, 3, 3), this model's "
                             f"has filters={eb_filters}; its module-by-module forward (model(y_cur, y_conditioned)) and autograd work")
        self.has_tpm, self.has_spm, self.residual = has_tpm, has_spm, residual
        L = lambda mod: _Layer(mod, "conv", self)
        D = lambda mod: _Layer(mod, "deconv", self)
        self.HE = [L(model.HE[0]), L(model.HE[2]), L(model.HE[4])]
        self.HD = [D(model.HD[0]), D(model.HD[2]), L(model.HD[4])]
        self.TPM = [L(model.TPM[0]), L(model.TPM[2]), L(model.TPM[4])] if has_tpm else None
        self.CTX = L(model.context_prediction) if has_spm else None
        self.EPM = [L(model.EPM[0]), L(model.EPM[2]), L(model.EPM[4])]
        self.nprior = 1 + int(has_tpm) + int(has_spm)
        self.layers = self.HE + self.HD + (self.TPM or []) + ([self.CTX] if has_spm else []) + self.EPM
        # no input gradient is ever needed for the first layer of a chain fed by (detached) data
        for first in [self.HE[0]] + ([self.TPM[0]] if has_tpm else []) + ([self.CTX] if has_spm else []):
            first.need_dgrad = False
        self._pack_key = None
        self._side = {}
        self._checked = False
        self._dgrad_pack_event = None
        self._fwd32_pack_event = None
        #: backward ADDS into .grad (autograd's semantics; several backward passes between two zero_grad() calls accumulate).  An explicit
        #: schedule that produces every gradient exactly once per step sets it False for its backward: the producers then OVERWRITE
        #: (no clearing pass, no read of the old value: 144 MB less HBM traffic per P-frame step of the big model)
        self.accumulate_grads = True
        self._events = {}
        self._tail_cache = None             # (key, plan) of tail_plan
        self._tail_last = None              # the last group's event of the latest ordered tail: every group is done when it is
        self._tail_waited = set()           # (stream, group) pairs that have waited for that tail's events already
        self._select_fx3()

    def _select_fx3(self):
        """Which layers run on the fp16 kernels.  HE.0 and HD.4 are routed one by one; the TPM and EPM chains hand planes from
        layer to layer (and the EPM input gradient is read through channel views at multiples of P = 2 * Cin), so each chain is
        routed as a whole: fp16 only if EVERY layer of it is eligible (channel counts multiples of 32) and, for the EPM, the
        views are 32-aligned -- otherwise the whole chain stays on the fp32-MFMA kernels, which only need C % 4 == 0."""
        for l in self.layers:
            l.fx3 = self.use_fx3 and l.fx3_eligible()
            l.taps = 0
            l.fx3s = False
        if self.use_fx3 and self.use_fx3s:
            # the hyper path's strided faces; each needs its neighbour's planes (HE.0 -> HE.2 -> HE.4, HD.4 -> HD.2 -> HD.0)
            if self.HE[0].fx3 and self.HE[1].fx3s_eligible():
                self.HE[1].fx3s = True
                self.HE[2].fx3s = self.HE[2].fx3s_eligible() and self.HE[1].K % 32 == 0
            if self.HD[2].fx3 and self.HD[1].fx3s_eligible():
                self.HD[1].fx3s = True
                self.HD[0].fx3s = self.HD[0].fx3s_eligible() and self.HD[1].C % 32 == 0
        if self.use_fx3t and self.use_wg3:
            for l in self.HE[1:] + self.HD[:2]:
                l.fx3t = l.fx3t_eligible()
            # planes travel down each chain: all of a chain's stride-2 layers or none
            if not (self.HE[1].fx3t and self.HE[2].fx3t and self.HE[0].fx3):
                self.HE[1].fx3t = self.HE[2].fx3t = False
            if not (self.HD[0].fx3t and self.HD[1].fx3t and self.HD[2].fx3):
                self.HD[0].fx3t = self.HD[1].fx3t = False
        if self.has_spm and self.use_fx3 and self.use_ctx3 and self.CTX.fx3_masked_eligible():
            self.CTX.fx3 = True
            self.CTX.taps = F.masked_live_taps(self.CTX.R, self.CTX.R, "B" if self.CTX.masked & 4 else "A")
        P = self.HE[0].C                                # HE.0 reads cat(y_cur, y_cond): its C is 2 * Cin = P
        for group, need_aligned in ((self.TPM, False), (self.EPM, True)):
            if group and not (all(l.fx3 for l in group) and (not need_aligned or P % 32 == 0)):
                for l in group:
                    l.fx3 = False
        for l in self.layers:
            # weight gradients take whatever planes the forward / input-gradient route left behind (_Layer.weight_grad falls back to
            # the fp32 kernel when there are none), so they follow the layer's own eligibility
            l.wg3 = self.use_fx3 and self.use_wg3 and l.wg3_eligible()
            l.set_faces()

    #: forward and input-gradient of the stride-1 layers (TPM, HE.0, HD.4, EPM) on the fp16 matrix cores: three fp16 products per fp32 product on operands split into two scaled fp16 planes, ~2^-21 relative per product (tests: 1e-4 gates; measured 0.4-1.6e-6 of max per layer against fp64)
    #: (three fp16 MFMAs per fp32 product, csrc/conv_f16x3.hip); STEM_ENGINE_F16X3=0 keeps every layer on the fp32-MFMA kernels
    use_fx3 = _Switch("engine_f16x3")
    #: the entropy glue (prologue, Gaussian backward) records the maxima of the fp32 tensors it writes, so that their fp16 splits
    #: skip the maximum pass (four launches per P-frame step); STEM_ENGINE_RECORDS=0: every split measures its input itself
    use_records = _Switch("engine_records")
    #: the strided-convolution faces of the hyper path's stride-2 layers (HE.2 / HE.4 forward, HD.2 / HD.0 input gradient) on the
    #: general fp16 kernel; STEM_ENGINE_STRIDED_F16X3=0: igemm.hip
    use_fx3s = _Switch("engine_strided_f16x3")
    #: ... and their TRANSPOSED faces (HD.0 / HD.2 forward, HE.2 / HE.4 input gradient: one launch over the four sub-pixel phases)
    #: plus the four layers' weight gradients (per-tap kernel, strided gather); STEM_ENGINE_TRANSPOSED_F16X3=0: igemm.hip / wgrad.hip
    use_fx3t = _Switch("engine_transposed_f16x3")
    #: the masked context convolution's forward on the same kernel over its live taps; STEM_ENGINE_CTX_F16X3=0: igemm.hip
    use_ctx3 = _Switch("engine_ctx_f16x3")
    #: ... and their weight gradients (csrc/wgrad_f16x3.hip); STEM_ENGINE_WGRAD_F16X3=0 keeps those on wgrad.hip
    use_wg3 = _Switch("engine_wgrad_f16x3")

    #: weight gradients (wgrad + bias column sums + unpack + the data-parallel exchange hook) run on their own stream
    #: and overlap the latency-bound parts of the dgrad chain; set False to keep everything on the compute stream
    overlap_wgrad = _Switch("engine_overlap")

    #: the next forward's weight packing is split: forward-role copies on the compute stream (the forward waits for them), the
    #: input-gradient copies on a weight-gradient stream (only backward waits): 22.48-22.62 ms against 22.67-22.82 ms per bench
    #: step; STEM_ENGINE_SPLIT_PACK=0: one launch each as before
    split_pack = _Switch("engine_split_pack")

    def side_stream(self, device, lane=0):
        if not self.overlap_wgrad or device.type != "cuda" or lane < 0:
            return None
        st = self._side.get(lane)
        if st is None or st.device != device:
            st = self._side[lane] = F.make_stream(device, "side")
        return st

    #: the hyper path (HE -> bottleneck -> HD) and the temporal / spatial priors are independent until the entropy-parameter
    #: network joins them: the hyper path runs on its own stream in forward and backward so that the ramp-up / drain of its
    #: small launches overlaps the other branch's kernels (30.90 -> 30.75 ms per bench step; STEM_ENGINE_BRANCH=0 disables)
    branch_streams = _Switch("engine_branch")

    def _branch(self, device, which=0):
        if not self.branch_streams or device.type != "cuda":
            return None
        bs = getattr(self, "_bstreams", None)
        if bs is None:
            bs = self._bstreams = {}
        st = bs.get(which)
        if st is None or st.device != device:
            st = bs[which] = F.make_stream(device, "branch")
        return st

    def ensure_packed(self, block_max=None, split=True):
        """(Re)build every layer's packed weight copies with ONE kernel launch when any weight changed.  Inside
        StemEngine.forward the check has already run for the whole schedule (`_checked`).
        split=False: every launch on the current stream, whatever `split_pack` says (a caller that orders all later work after
        the current stream and cannot wait for the events of the side streams: tape.TapedPFrameStep).
        block_max = (maxima, flat): the per-chunk maxima an optimiser pass just left for the flat parameter buffer `flat`
        (optim.step(block_max=True)); the fp16 images of weights inside that buffer take their scales from them instead of a
        maximum launch.  Only meaningful in the call that directly follows that optimiser step."""
        if self._checked:
            return
        if self._weights_key() == self._pack_key:
            return
        self._drop_tail()                 # whatever an ordered tail still holds on the weight-gradient stream comes first
        have = [l.wp_fwd if l.faces[0].kind == "f32" else l.wp6_fwd for l in self.layers]        # the forward face's copy of each layer
        if any(h is None or h.device != l.mod.weight.device for h, l in zip(have, self.layers)):
            for l in self.layers:
                l.alloc_packs(l.mod.weight.device)
        dev = self.layers[0].mod.weight.device
        if block_max is not None and self.pack_pair and self._pack_pairs(*block_max):
            self._pack_key = self._weights_key()
            return
        side = self.side_stream(dev) if split and self.split_pack and not torch.cuda.is_current_stream_capturing() else None
        if not split:
            # ... and after whatever the engine's own streams still hold: an earlier packing launch may be among it
            for st in list(self._side.values()) + list(getattr(self, "_bstreams", {}).values()):
                F.stream_wait(F.cur_stream(dev), st)
            self._dgrad_pack_event = None
        roles = ((0, 1), (1, 2)) if side is not None else ((0, 2),)
        for lo, hi in roles:                     # descriptor 0 of a layer = forward role, descriptor 1 = input-gradient role
            on_side = side is not None and lo == 1
            if on_side:
                F.stream_wait(side, F.cur_stream(dev))      # the optimiser step that changed the weights
            with F.on_stream(side if on_side else None):
                both = [l.role_descs(r) for l in self.layers for r in range(lo, hi)]
                descs = [d for a, _ in both for d in a]
                descs6 = [d for _, b in both for d in b]
                if descs6 and block_max is not None:
                    ch = F.adam_chunk()
                    for d in descs6:
                        _attach_block_maxima(d, d.N * d.C * d.R * d.S, *block_max, ch)
                if descs6:                        # the forward's first kernels (HE.0, TPM.0, the context model) wait for these
                    F.pack_weights_f16x2_multi((_lib.F16PackDesc * len(descs6))(*descs6))
                # the fp32 copies of the forward role (the transposed hyper-decoder layers: consumed on the hyper branch, half a
                # forward later) are packed on that branch's stream, off the compute stream's optimiser -> forward chain
                bs = self._branch(dev) if (descs and side is not None and not on_side and lo == 0 and hi == 1) else None
                if descs and bs is not None:
                    F.stream_wait(bs, F.cur_stream(dev))
                    with F.on_stream(bs):
                        F.pack_weights_multi((_lib.PackDesc * len(descs))(*descs))
                        # one event object for the lifetime of the engine: a launch tape replays the record and the wait on it
                        self._fwd32_pack_event = self._events.setdefault("fwd32", torch.cuda.Event())
                        F.event_record(self._fwd32_pack_event, bs)
                elif descs:
                    F.pack_weights_multi((_lib.PackDesc * len(descs))(*descs))
                    if not on_side:
                        self._fwd32_pack_event = None
                if on_side:
                    self._dgrad_pack_event = self._events.setdefault("dgrad", torch.cuda.Event())
                    F.event_record(self._dgrad_pack_event, side)
        # masked == 2 zeroed taps of the context weight in place: refresh its version in the key
        self._pack_key = self._weights_key()

    def _weights_key(self):
        """changes whenever a weight of the schedule was written or moved: the packed copies are then stale"""
        return tuple((_layers.weight_epoch(l.mod.weight), l.mod.weight._version, l.mod.weight.data_ptr()) for l in self.layers)

    #: after an optimiser pass that left chunk maxima, both images of every layer come from ONE launch that reads each weight once
    #: (F.pack_weights_f16x2_pair_multi) on the compute stream, instead of one launch per role (the input-gradient role on the
    #: weight-gradient stream, under the forward).  STEM_ENGINE_PACK_PAIR=0: one launch per role as in round 4
    pack_pair = _Switch("engine_pack_pair")

    def _pack_pairs(self, maxima, flat):
        """the pair pack of every layer, if every layer's images are fp16 transposes of its tensor and every tensor lies inside the
        flat buffer the optimiser pass measured; else False (the per-role path runs)"""
        descs = [l.pair_desc() for l in self.layers]
        if any(d is None for d in descs):
            return False
        ch = F.adam_chunk()
        if not all(_attach_block_maxima(d, d.A * d.B * d.R * d.S, maxima, flat, ch) for d in descs):
            return False
        F.pack_weights_f16x2_pair_multi((_lib.F16PairDesc * len(descs))(*descs))
        self._dgrad_pack_event = None
        return True

    #: the optimiser tail of the fused P-frame step in the order the next forward first uses the layers (tail_plan / run_tail): the
    #: forward starts after the first group, the rest of the optimiser pass and of the packing runs under its first kernels on the
    #: weight-gradient stream.  STEM_ENGINE_TAIL_ORDERED=0: one optimiser pass, one pair pack, the forward behind both
    tail_ordered = _Switch("engine_tail_ordered")

    #: optional callable(): invoked with the weight-gradient stream current just before the later groups of an ordered tail are
    #: enqueued on it (a test delays the stream there: a consumer that does not wait for its group's event then reads stale images)
    tail_hook = None

    _TailGroup = collections.namedtuple("_TailGroup", "index table descs layers event")

    def _tail_order(self):
        """the layers by first use in the forward: TPM.0 / HE.0 open it, the stride-2 hyper encoder and the temporal prior follow
        side by side, then the hyper decoder, the context model and the entropy-parameter network.  Three groups: HE.2 / TPM.2
        apart from HE.4 / TPM.4 (four groups: three more entries for the host in front of the next forward's first launch)
        measured no better, 0.12 against 0.15 ms per bench step gained over the single pass"""
        tpm = self.TPM or [None] * 3
        groups = [[tpm[0], self.HE[0]], [self.HE[1], tpm[1], self.HE[2], tpm[2]], self.HD + [self.CTX] + self.EPM]
        return [[l for l in g if l is not None] for g in groups]

    def tail_plan(self, opt):
        """The ordered optimiser tail for `opt` (optim.FusedClipAdam with chunk maxima), or None when it does not apply (a layer with an
        fp32 face, a weight outside the flat buffer, more chunk ranges than a table holds): the groups of _tail_order, each one table
        of chunk ranges for stem_adam_step_bmax_ranges and the pair-pack descriptors of its layers.  Group 0 also holds every
        parameter that is no layer's weight (biases, the bottleneck's tensors: forward kernels read them in place).  A chunk that
        touches tensors of several groups belongs to the EARLIEST of them, so every chunk covering a tensor is final when the
        tensor's group packs it and its scale -- the maximum over those chunks -- is the number one whole pass leaves."""
        flat, maxima = opt.flat, opt.block_maxima
        if any((l.wp_fwd if l.faces[0].kind == "f32" else l.wp6_fwd) is None for l in self.layers):
            return None
        key = (flat.data.data_ptr(), flat.numel, maxima.data_ptr(), tuple(flat.offsets),
               tuple((l.mod.weight.data_ptr(), l.faces, l.taps, l.wp6_fwd.data_ptr() if l.wp6_fwd is not None else 0,
                      l.wp6_dgrad.data_ptr() if l.wp6_dgrad is not None else 0) for l in self.layers))
        if self._tail_cache is not None and self._tail_cache[0] == key:
            return self._tail_cache[1]
        self._tail_cache = (key, self._build_tail_plan(flat, maxima))
        return self._tail_cache[1]

    def _build_tail_plan(self, flat, maxima, max_ranges=40):
        ch = F.adam_chunk()
        order = self._tail_order()
        group_of = {id(l.mod.weight): gi for gi, g in enumerate(order) for l in g}
        in_flat = {id(p) for p in flat.params}
        if any(id(l.mod.weight) not in in_flat for l in self.layers):
            return None
        all_ranges = tail_chunk_ranges([(off, p.numel(), group_of.get(id(p), 0)) for p, off in zip(flat.params, flat.offsets)],
                                       flat.numel, ch, len(order))
        plan = []
        for gi, layers in enumerate(order):
            ranges = all_ranges[gi]
            descs = [l.pair_desc() for l in layers]
            if len(ranges) > max_ranges or any(d is None for d in descs):
                return None
            if not all(_attach_block_maxima(d, d.A * d.B * d.R * d.S, maxima, flat.data, ch) for d in descs):
                return None
            if not layers and not ranges:
                continue
            if not layers and plan:           # chunks without a layer of their own (cannot happen past group 0): to the group before
                return None
            plan.append(self._TailGroup(len(plan), F.adam_ranges(ranges), (_lib.F16PairDesc * len(descs))(*descs) if descs else None, layers,
                                        self._events.setdefault(("tail", len(plan)), torch.cuda.Event())))
        return plan

    def run_tail(self, plan, adam):
        """Issue the groups of `plan`; adam(table): the optimiser's launch over one table of chunk ranges on the current stream.
        Group 0 runs on the current stream, the others on the weight-gradient stream behind group 0's optimiser launch (a tensor
        of a later group may share a chunk with one of group 0), each followed by its event: _Layer.forward / input_grad wait for
        it on their own stream before the layer's first launch of the next step."""
        dev = self.layers[0].mod.weight.device
        main, side = F.cur_stream(dev), self.side_stream(dev)
        adam(plan[0].table)
        F.stream_wait(side, main)
        if plan[0].descs is not None:
            F.pack_weights_f16x2_pair_multi(plan[0].descs)
        with F.on_stream(side):
            if self.tail_hook is not None:
                F.tape_py(self.tail_hook)
            for g in plan[1:]:
                adam(g.table)
                F.pack_weights_f16x2_pair_multi(g.descs)
                F.event_record(g.event, side)
        self.mark_tail(plan)
        self._dgrad_pack_event = None
        self._pack_key = self._weights_key()

    def mark_tail(self, plan):
        """the host-side state run_tail(plan) leaves (a launch tape that replayed one calls this: trainer.FusedPFrameStep.after_replay)"""
        self._tail_waited.clear()
        for l in self.layers:
            l.tail_event = None
        for g in plan[1:]:
            for l in g.layers:
                l.tail_event, l.tail_group = g.event, g.index
        self._tail_last = plan[-1].event if len(plan) > 1 else None

    def _wait_tail(self, layer):
        """a consumer of `layer`'s images: the current stream waits for the layer's group of the ordered tail, once per stream"""
        st = F.cur_stream()
        key = (st.cuda_stream, layer.tail_group)
        if key not in self._tail_waited:
            self._tail_waited.add(key)
            F.event_wait(st, layer.tail_event)

    def join_tail(self):
        """order the current stream after every group of the latest ordered tail (a reader or writer of the parameters themselves)"""
        if self._tail_last is not None:
            F.event_wait(F.cur_stream(), self._tail_last)

    def _drop_tail(self):
        """the images are about to be packed another way: the current stream goes behind the ordered tail, whose events retire"""
        self.join_tail()
        self._tail_last = None
        self._tail_waited.clear()
        for l in self.layers:
            l.tail_event = None

    def unpack_all(self):
        for lane in sorted({l.lane for l in self.layers}):
            self._group_ready([l for l in self.layers if l.lane == lane], [])

    #: optional callable(list_of_parameters): invoked during backward as soon as the gradients of a module group
    #: (EPM, context_prediction, TPM, HD + entropy_bottleneck, HE -- the order backward produces them) are final,
    #: so a data-parallel reducer can start exchanging that slice while the rest of backward still runs
    grad_ready_hook = None

    def _group_ready(self, layers, extra_params):
        dev = layers[0].mod.weight.device
        side = self.side_stream(dev, layers[0].lane)
        if side is None:
            return self._group_ready_on_stream(layers, extra_params)
        # extra_params (entropy-bottleneck gradients) were produced on the compute stream: order them before the hook
        F.stream_wait(side, F.cur_stream(dev))
        with F.on_stream(side):
            self._group_ready_on_stream(layers, extra_params)

    def _group_ready_on_stream(self, layers, extra_params):
        bdescs = [l.pending_bias for l in layers if getattr(l, "pending_bias", None) is not None]
        for l in layers:
            l.pending_bias = None
        if bdescs:
            F.bias_grad_final_multi(bdescs)
        descs = [l.unpack_desc() for l in layers if l.pending is not None]
        if descs:
            arr = (_lib.UnpackDesc * len(descs))(*descs)
            F.unpack_wgrads_multi(arr)
        if self.grad_ready_hook is not None:
            params = [p for l in layers for p in (l.mod.weight, l.mod.bias) if p is not None] + list(extra_params)
            if params:
                hook = self.grad_ready_hook
                F.tape_py(lambda: hook(params))          # torch.distributed calls: a launch tape re-runs them at this point

    def join_side_stream(self):
        for st in self._side.values():
            F.stream_wait(F.cur_stream(st.device), st)

    def _wait_fwd32_packs(self):
        """a consumer of a forward-role fp32 weight copy: order it after the packing on the hyper branch's stream (a no-op
        for the hyper branch itself, which runs on that stream)"""
        if self._fwd32_pack_event is not None:
            F.event_wait(F.cur_stream(), self._fwd32_pack_event)

    def _wait_dgrad_packs(self):
        """backward's first consumer of an input-gradient weight copy: order it after the side-stream packing"""
        if self._dgrad_pack_event is not None:
            F.event_wait(F.cur_stream(), self._dgrad_pack_event)
            self._dgrad_pack_event = None

    # -------------------------------------------------------------------------------------------
    def forward(self, y_cur, y_cond, training: bool, rate_coef=None):
        """rate_coef = (coef, scale) selects the fused training glue (training only): the elementwise work between the
        convolutions runs as 4 kernels that also produce dlik = coef / lik and (y_bpp, z_bpp, loss) = scale * sum log2 lik,
        i.e. EMLoss forward AND backward (utils.py:18-27): `k` then carries "dlik_y", "dlik_z", "loss3"."""
        self.ensure_packed()
        self._checked = True          # weights cannot change inside one forward: skip the per-layer checks
        try:
            return self._forward(y_cur, y_cond, training, rate_coef)
        finally:
            self._checked = False

    @staticmethod
    def _chain_forward(layers, a, out=None, planes=True):
        """a chain of convolutions with leaky ReLUs between them over the _Act `a`; the last one writes `out` (a channel slice of
        the EPM input) if given.  -> [a, output of layer 0, ...]: an epilogue writes planes when the next layer reads them.
        planes=False: no epilogue writes planes, every layer splits its fp32 input itself, which is codec._chain's arithmetic
        (an epilogue scales its planes by a bound of |output|, a split by the measured maximum: the low planes differ)"""
        acts = [a]
        for i, l in enumerate(layers):
            nxt = layers[i + 1] if i + 1 < len(layers) else None
            acts.append(l.forward(acts[-1], F.ACT_LRELU if nxt else F.ACT_NONE, out=None if nxt else out,
                                  planes=planes and nxt is not None and nxt.faces[0].kind != "f32"))
        return acts

    @staticmethod
    def _chain_backward(layers, xs, dy, planes=False):
        """from the last layer to the first: weight gradient of layer i from its input xs[i] and `dy`, then `dy` through layer i
        (the leaky-ReLU derivative at xs[i] folded in for i > 0).  -> the gradient of xs[0], with planes if `planes` and the route
        can write them; None when the first layer has no input gradient.  Where the input gradient reads planes of dy they are made
        before the weight gradient (with dy's scale record), so that both read the same ones."""
        for i in range(len(layers) - 1, -1, -1):
            l = layers[i]
            if l.faces[1] is not None and l.faces[1].kind != "f32":
                dy.planes()
            l.weight_grad(xs[i], dy)
            if l.faces[1] is None:
                return None
            dy = l.input_grad(dy, xact=xs[i].x if i else None, x_shape=xs[i].x.shape,
                              planes=layers[i - 1].reads_dy_planes(xs[i - 1]) if i else planes)
        return dy

    def _forward(self, y_cur, y_cond, training: bool, rate_coef=None):
        m = self.m
        yc, yd = F.to_nhwc(y_cur.detach()), F.to_nhwc(y_cond.detach())
        B, Cin, H, W = yc.shape
        dev = yc.device
        eb, gc = m.entropy_bottleneck, m.gaussian_conditional
        fused = rate_coef is not None
        assert not fused or training, "the fused glue is the TRAINING forward"
        k = {}
        target = t_hat = y_hat = None
        # the eval forward of a model WITHOUT a spatial prior returns y_hat = round(y - means) + means, the very tensor its decoder
        # rebuilds (codec.stem_decompress): its chains run codec._chain's arithmetic so that the two means are the same floats
        ep = training or self.has_spm
        rec = {}    # scale records left by the producers of fp32 tensors that are split for the fp16 kernels below
        if fused:
            # one kernel: he_in = [y_cur | y_cond], target, t_hat = target + noise, y_hat = t_hat (+ y_cond); it also records
            # max |y_cur|, |y_cond| and max |t_hat| per workgroup: the splits of he_in, y_cond and t_hat need no maximum pass
            slot = gc._noise_slot(yc) if self.has_spm else {}
            he_in, target, t_hat, y_hat = F.prior_prologue(yc, yd, self.residual, True, self.has_spm, records=rec if self.use_fx3 and self.use_records else None, **slot)
        else:
            # hyper encoder on cat(y_cur, y_cond): the two halves are written into one buffer
            he_in = F.empty_nhwc(B, 2 * Cin, H, W, dev)
            F.copy_channels(yc, he_in[:, :Cin])
            F.copy_channels(yd, he_in[:, Cin:])
        P = 2 * Cin
        epm_in = F.empty_nhwc(B, self.nprior * P, H, W, dev)
        o_tp, o_hp = (0, P) if self.has_tpm else (None, 0)
        o_ctx = o_hp + P
        bs = self._branch(dev)
        main = F.cur_stream(dev) if bs is not None else None
        if bs is not None:
            F.stream_wait(bs, main)
        acts = k["acts"] = {}             # every activation backward reads, with the planes the forward made of it
        acts["he_in"] = _Act(he_in, rec=rec.get("in"))
        acts["yd"] = _Act(yd, rec=rec.get("in"))                     # max(|y_cur|, |y_cond|) bounds y_cond
        ctx_split_done = None
        if self.has_spm and fused:
            acts["t_hat"] = _Act(t_hat, rec=rec.get("t_hat"))
            if self.CTX.fx3 and rec.get("t_hat") is not None and self.side_stream(dev) is not None:
                # t_hat exists since the prologue and the context model runs behind the TPM chain: its planes are made meanwhile on the
                # weight-gradient stream, which has nothing to do during the forward (one launch less between TPM.4 and the context model)
                side = self.side_stream(dev)
                F.stream_wait(side, F.cur_stream(dev))
                with F.on_stream(side):
                    acts["t_hat"].planes()
                    ctx_split_done = self._events.setdefault("ctx_split", torch.cuda.Event())
                    F.event_record(ctx_split_done, side)
                t_hat.record_stream(side)

        if fused and self.HE[0].fx3 and self.has_tpm and self.TPM[0].fx3 and Cin % 32 == 0 and rec.get("in") is not None:
            # he_in = [y_cur | y_cond] and the TPM chain's input y_cond share ONE planes tensor (same record: max(|y_cur|, |y_cond|)):
            # one split on the compute stream, the TPM chain reads its second half as a channel view, the hyper branch (which waits
            # for this stream anyway) the whole -- a launch less, the same values
            acts["yd"] = _Act(yd, acts["he_in"].planes().channels(Cin, 2 * Cin))
            if bs is not None:
                F.stream_wait(bs, main)

        # the TPM chain is enqueued ahead of the hyper branch's ~14 launches: it is the forward's critical path
        tp0 = tp2 = None
        if self.has_tpm:
            _, acts["tp0"], acts["tp2"], _ = self._chain_forward(self.TPM, acts["yd"], out=epm_in[:, o_tp:o_tp + P], planes=ep)
            tp0, tp2 = acts["tp0"].x, acts["tp2"].x
        with F.on_stream(bs):
            _, acts["he0"], acts["he2"], z = self._chain_forward(self.HE, acts["he_in"], planes=ep)
            z = z.x
            pack = F.eb_pack(eb._tensors14())
            if fused:
                if self.HD[0].fx3t and self.use_records:         # the kernel leaves max |z_hat| for the split below: no maximum pass
                    z_hat, lik_z, k["dlik_z"], part_z, rec["z_hat"] = F.eb_forward_train(z, pack, rate_coef[0], bound=eb._lik_bound, record=True,
                                                                                         **eb._noise_slot(z))
                else:
                    z_hat, lik_z, k["dlik_z"], part_z = F.eb_forward_train(z, pack, rate_coef[0], bound=eb._lik_bound, **eb._noise_slot(z))
            elif training:
                z_hat, lik_z = F.eb_forward(z, pack, noise=eb._noise_like(z))
            else:
                z_hat, lik_z = F.eb_forward(z, pack, medians=eb._medians_vec())
            # hyper decoder; its last conv writes the `hp` slice of the EPM input
            acts["z_hat"], acts["hd0"], acts["hd2"], _ = self._chain_forward(self.HD, _Act(z_hat, rec=rec.get("z_hat")), out=epm_in[:, o_hp:o_hp + P], planes=ep)
        if not fused:
            target = F.sub(yc, yd) if self.residual else (yc if F.nhwc_ld(yc) == Cin else F.copy_channels(yc, F.empty_nhwc(B, Cin, H, W, dev)))
        if self.has_spm:
            # gaussian_conditional.quantize(target, "noise" | "dequantize") with no means (:570-572, :853-855)
            if not fused:
                t_hat = F.add(target, gc._noise_like(target)) if training else F.round_(target)
                acts["t_hat"] = _Act(t_hat)
            if ctx_split_done is not None:
                F.event_wait(F.cur_stream(dev), ctx_split_done)
            # context_prediction(t_hat) -> its channel slice of the EPM input (spatiotemporalpriors.py:857): on the fp16 kernel over
            # the live taps of the mask (the planes of t_hat stay for the weight gradient), else on igemm.hip's masked form
            self.CTX.forward(acts["t_hat"], out=epm_in[:, o_ctx:o_ctx + P])
        if bs is not None:
            F.stream_wait(main, bs)
        acts["epm_in"], acts["e0"], acts["e2"], gp = self._chain_forward(self.EPM, _Act(epm_in), planes=ep)
        gp = gp.x                                                    # [B, 2*Cin, H, W] = scales | means
        scales, means = gp[:, :Cin], gp[:, Cin:]
        if fused:
            # the GaussianConditional's backward in the same launch (d loss / d likelihood = coef / lik is known here): backward()
            # uses it when it is handed this very dlik_y
            dgp = F.empty_nhwc(B, 2 * Cin, H, W, dev)
            gc_out, lik_y, k["dlik_y"], part_y, k["qg"] = F.gc_forward_train(
                target, scales, means, rate_coef[0], scale_bound=gc._scale_bound, lik_bound=gc._lik_bound,
                backward=(dgp[:, :Cin], dgp[:, Cin:]), record=self.EPM[0].fx3 and self.use_records, **gc._noise_slot(target))
            k["dgp"] = dgp
            k["loss3"] = F.em_loss_finalize(part_y, part_z, rate_coef[1])
            if not self.has_spm:
                y_hat = gc_out
        else:
            noise = gc._noise_like(target) if training else None
            gc_out, lik_y = F.gc_forward(target, scales, means, noise=noise, scale_bound=gc._scale_bound, lik_bound=gc._lik_bound)
            if self.has_spm:
                y_hat = F.add(t_hat, yd if F.nhwc_ld(yd) == Cin else F.copy_channels(yd, F.empty_nhwc(B, Cin, H, W, dev))) if self.residual else t_hat
            else:
                y_hat = gc_out
        k.update(he_in=he_in, he0=acts["he0"].x, he2=acts["he2"].x, z_hat=z_hat, pack=pack, hd0=acts["hd0"].x, hd2=acts["hd2"].x,
                 epm_in=epm_in, tp0=tp0, tp2=tp2, yd=yd, t_hat=t_hat, e0=acts["e0"].x, e2=acts["e2"].x, gp=gp, gc_out=gc_out,
                 offs=(o_tp, o_hp, o_ctx), P=P, Cin=Cin)
        return y_hat, lik_y, lik_z, k

    # -------------------------------------------------------------------------------------------
    def eval_rate(self, y_cur, y_cond, num_pixels, acc=None, weight=1.0):
        """The eval-mode forward with its EMLoss value, on the fused validation glue (include/stem_validation.h): the step of a
        validation pass (stem/trainSTEM.py:280-287).  -> (y_hat, lik_y, lik_z, loss3): the three tensors are forward(y_cur, y_cond,
        False)'s, bit for bit; loss3 = fp64 (y_bpp, z_bpp, loss) with the -1 / num_pixels normalisation of utils.py:18-27.
        acc: an fp64 [4] device tensor that receives acc[0..2] += weight * loss3, acc[3] += weight (one is made and dropped when None).
        No noise is drawn and no noise offset moves; nothing syncs with the host."""
        self.ensure_packed()
        self._checked = True
        try:
            return self._eval_rate(y_cur, y_cond, num_pixels, acc, weight)
        finally:
            self._checked = False

    def _eval_rate(self, y_cur, y_cond, num_pixels, acc, weight):
        # the schedule of _forward(training=False) with its elementwise work regrouped: prologue (he_in, target, round(target), y_hat),
        # bottleneck + rate, Gaussian + rate, loss + running sum.  No scale records: every split measures its own input, as there
        m = self.m
        yc, yd = F.to_nhwc(y_cur.detach()), F.to_nhwc(y_cond.detach())
        B, Cin, H, W = yc.shape
        dev = yc.device
        eb, gc = m.entropy_bottleneck, m.gaussian_conditional
        ep = self.has_spm                     # _forward's `training or self.has_spm`: without a spatial prior, codec._chain's arithmetic
        he_in, target, t_hat, y_hat = F.prior_prologue(yc, yd, self.residual, False, self.has_spm, records=None)
        P = 2 * Cin
        epm_in = F.empty_nhwc(B, self.nprior * P, H, W, dev)
        o_tp, o_hp = (0, P) if self.has_tpm else (None, 0)
        o_ctx = o_hp + P
        bs = self._branch(dev)
        main = F.cur_stream(dev) if bs is not None else None
        if bs is not None:
            F.stream_wait(bs, main)
        if self.has_tpm:
            self._chain_forward(self.TPM, _Act(yd), out=epm_in[:, o_tp:o_tp + P], planes=ep)
        with F.on_stream(bs):
            z = self._chain_forward(self.HE, _Act(he_in), planes=ep)[-1].x
            z_hat, lik_z, part_z = F.eb_forward_eval_rate(z, F.eb_pack(eb._tensors14()), eb._medians_vec())     # _forward's eval call
            self._chain_forward(self.HD, _Act(z_hat), out=epm_in[:, o_hp:o_hp + P], planes=ep)
        if self.has_spm:
            self.CTX.forward(_Act(t_hat), out=epm_in[:, o_ctx:o_ctx + P])
        if bs is not None:
            F.stream_wait(main, bs)
            for t in (lik_z, part_z):
                t.record_stream(main)         # allocated on the branch stream, read (and freed) on this one
        gp = self._chain_forward(self.EPM, _Act(epm_in), planes=ep)[-1].x
        gc_out, lik_y, part_y = F.gc_forward_eval_rate(target, gp[:, :Cin], gp[:, Cin:], scale_bound=gc._scale_bound, lik_bound=gc._lik_bound)
        if acc is None:
            acc = torch.zeros(4, dtype=torch.float64, device=dev)
        loss3 = F.em_loss_accumulate(part_y, part_z, -1.0 / num_pixels, acc, weight=weight)
        return (y_hat if self.has_spm else gc_out), lik_y, lik_z, loss3

    # -------------------------------------------------------------------------------------------
    def backward(self, k, dlik_y, dlik_z):
        """Parameter gradients of a scalar that depends on (lik_y, lik_z), ADDED into .grad as autograd does (the
        training loop zeroes them before every backward, stem/trainSTEM.py:203; a slot that does not exist yet starts
        at zero), so several backward passes between two zero_grad() calls accumulate -- the same semantics as the
        layer-wise Functions of the variable-rate models (layers.py)."""
        m = self.m
        gc = m.gaussian_conditional
        Cin, P = k["Cin"], k["P"]
        o_tp, o_hp, o_ctx = k["offs"]
        gp, acts = k["gp"], k["acts"]
        B, _, H, W = gp.shape
        self._wait_dgrad_packs()
        if k.get("dgp") is not None and dlik_y is k.get("dlik_y"):          # computed by the fused forward glue
            dgp, qg = k["dgp"], k["qg"]
        else:
            dgp = F.empty_nhwc(B, 2 * Cin, H, W, gp.device)
            qg = F.gc_backward(k["gc_out"], gp[:, :Cin], gp[:, Cin:], dlik_y, dgp[:, :Cin], dgp[:, Cin:], dy=None,
                               scale_bound=gc._scale_bound, lik_bound=gc._lik_bound, record=self.EPM[0].fx3 and self.use_records)
        # EPM (1x1 chain); the prior branches read 32-aligned channel views of its input gradient (and of its planes)
        dpri = self._chain_backward(self.EPM, [acts["epm_in"], acts["e0"], acts["e2"]], _Act(dgp, rec=qg), planes=True)
        self._group_ready(self.EPM, [])
        bs = self._branch(gp.device)
        main = F.cur_stream(gp.device)

        if bs is not None:                 # the hyper chain depends on the EPM input gradient only: its point on the compute stream
            epm_done = self._events.setdefault("bwd_epm", torch.cuda.Event())
            F.event_record(epm_done, main)
        # spatial prior: weight gradient of all 25 taps, no input gradient (its input is data + noise)
        if self.has_spm:
            self._chain_backward([self.CTX], [acts["t_hat"]], dpri.channels(o_ctx, o_ctx + P))
            self._group_ready([self.CTX], [])
        if self.has_tpm:
            # with a hyper branch stream, the chain's weight gradients (~300 us of the ~900 us the weight-gradient stream carries per
            # P-frame step) go on the compute stream, behind its own input gradients: that stream is otherwise idle by then, while the
            # weight-gradient stream finished last by ~250 us (profiles/r05_gantt_palone.txt).  lane -1 = "the stream backward runs on"
            for l in self.TPM:
                l.lane = -1 if bs is not None else 0
            self._chain_backward(self.TPM, [acts["yd"], acts["tp0"], acts["tp2"]], dpri.channels(o_tp, o_tp + P))
            self._group_ready(self.TPM, [])
        if bs is None:
            self._backward_hyper(k, dpri.channels(o_hp, o_hp + P), dlik_z)
        else:                              # hyper chain (HD -> bottleneck -> HE) on its own stream, enqueued behind the TPM chain
            F.event_wait(bs, epm_done)
            with F.on_stream(bs):
                self._backward_hyper(k, dpri.channels(o_hp, o_hp + P), dlik_z)
            F.stream_wait(main, bs)
        self.join_side_stream()          # gradients are complete for whatever the compute stream does next

    def _backward_hyper(self, k, dhp, dlik_z):
        """dhp: the gradient of the hyper decoder's slice of the EPM input (_Act)"""
        acts = k["acts"]
        # hyper decoder
        dz_hat = self._chain_backward(self.HD, [acts["z_hat"], acts["hd0"], acts["hd2"]], dhp).x
        # entropy bottleneck: d/dz = dz_hat + likelihood path; 58 parameter gradients per channel
        eb = self.m.entropy_bottleneck
        qdz = None
        if self.HE[2].fx3t and self.use_records:       # the kernel leaves max |dz| for the split in front of the hyper encoder's backward
            dz, dpack, qdz = F.eb_backward(k["z_hat"], k["pack"], dlik_z, dzhat_in=dz_hat, bound=eb._lik_bound, record=True)
        else:
            dz, dpack = F.eb_backward(k["z_hat"], k["pack"], dlik_z, dzhat_in=dz_hat, bound=eb._lik_bound)
        F.eb_unpack_grads(dpack, [_grad_of(p) for p in eb._tensors14()], accumulate=self.accumulate_grads)
        self._group_ready(self.HD, eb._tensors14())
        # hyper encoder
        self._chain_backward(self.HE, [acts["he_in"], acts["he0"], acts["he2"]], _Act(dz, rec=qdz))
        self._group_ready(self.HE, [])


class StemFunction(torch.autograd.Function):
    """Autograd node wrapping a whole STEM forward: inputs are the model parameters (so that
    `loss.backward()` reaches us), outputs (y_hat, lik_y, lik_z).  Parameter gradients are written
    directly into `.grad` by the engine and `None` is returned to autograd."""

    @staticmethod
    def forward(ctx, engine, training, y_cur, y_cond, *params):
        y_hat, lik_y, lik_z, k = engine.forward(y_cur, y_cond, training)
        ctx.engine, ctx.keep = engine, k
        ctx.mark_non_differentiable(y_hat)
        return y_hat, lik_y, lik_z

    @staticmethod
    def backward(ctx, _dy_hat, dlik_y, dlik_z):
        eng, k = ctx.engine, ctx.keep
        if k is None:
            raise RuntimeError("StemFunction: backward through this forward a second time -- its saved activations were "
                               "released by the first backward (retain_graph is not supported by the fused schedule; "
                               "run the forward again)")
        ctx.keep = None
        gp = k["gp"]
        B, _, H, W = gp.shape
        if dlik_y is None:
            dlik_y = torch.zeros_like(k["gc_out"])
        if dlik_z is None:
            dlik_z = torch.zeros_like(k["z_hat"])
        eng.backward(k, _dense(dlik_y), _dense(dlik_z))
        return (None,) * (4 + len(eng.m._engine_params))


def _dense(t):
    t = F.to_nhwc(t)
    if F.nhwc_ld(t) != t.shape[1]:
        t = F.copy_channels(t, F.empty_nhwc(*t.shape, t.device))
    return t
