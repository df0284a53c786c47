"""A stand-alone sequence codec over the frame container of bitstream.py: an encoder that writes a file and never decodes, and a decoder
that has nothing but that file and the two models.

    encode_sequence(imodel, stem, frames, out, gop=12, ...)     frames -> file; g_s never runs, no decompress is called
    decode_sequence(imodel, stem, src, write_to=None, ...)      file -> planar 4:2:0 frames (and the cropped x_hat tensors)
    python -m spatiotemporalentropymodel_amd.video encode|decode ...

evaluation.eval_gop / eval_sequence compress a frame and decompress it at once with the same objects, because the next P frame is
conditioned on the DECODED latents.  The encoder already holds those: the raster-order coding kernels leave the reconstruction in their
buffer, the one-shot coder has the symbols and the means (`return_y_hat=True` of codec.py's compress entry points).  So a sequence of N
frames costs N encodes here, not N encodes and N decodes, and every record is the bytes eval_gop produces for that frame: GOPs are
independent chains that advance side by side (evaluation.gop_schedule, the `*_each` entry points), transforms at batch 1.

File layout (all integers big-endian, as in bitstream.py):

    header   4s magic "STMV" | u8 version | u32 w | u32 h | u8 bit depth | u32 frames | u32 gop | u8 all_intra | u8 quality
             | u8 I-frame model id (bitstream.model_ids) | u16 N | u16 M | u32 fingerprint
             | u8 STEM class (index in STEM_CLASSES; 255: none, an all-intra file) | u16 N | u16 M | u32 fingerprint
    records  one per frame in display order, each written by bitstream.write_frame and read by bitstream.read_frame

Frame k is an I or a P frame by its index and `gop` (evaluation.gop_schedule's rule), so a record needs no type field.  Every record's
2-byte header names the I-FRAME model, also a P record's: the container's ids are the six zoo names, the STEM classes have none, and a P
frame is a frame of that image model's latent space -- its g_s turns the decoded latent into pixels.  An I record therefore is byte for
byte the record the reference's tool writes for that image.  Bit 7 of the second header byte marks wavefront symbol order
(bitstream.ORDER_BIT).  A record is skipped without parsing its strings, by the length prefixes (`record_ranges`): decoding
frames=(start, stop) touches only the GOPs that cover the range.

The fingerprint is zlib.crc32 over a model's state_dict in key order: each key's name, then the tensor's bytes (a masked convolution's
weight through its mask: `fingerprint`).  It covers the weights and the integer CDF tables (buffers of the entropy models): a decoder with other weights, or with tables rebuilt on another host's libm,
would decode garbage without noticing, so it refuses instead.  It is a check against mistakes, not against tampering.

Frames enter through functional.yuv420_to_rgb_padded (integer planes of a data.YUVSequence -> the padded fp32 frame, one kernel) and
leave through functional.rgb_window_to_yuv420 (the window of the padded x_hat -> integer planes, one kernel): no eager-torch pad, crop
or copy of a frame on the device.  The pixel-domain (stem_roi) models have a codec of their own: video_pixel.py.
"""
from __future__ import annotations

import io
import os
import struct
import sys
import zlib

import torch

from . import bitstream

MAGIC = b"STMV"
VERSION = 1
#: the P-frame model's index in the file header
STEM_CLASSES = ("SpatioTemporalPriorModelWithoutSPMTPM", "SpatioTemporalPriorModelWithoutSPM", "SpatioTemporalPriorModelWithoutTPM",
                "SpatioTemporalPriorModel", "SpatioTemporalPriorModel_Res")
NO_STEM = 255
_HEADER = struct.Struct(">4sBIIBIIBB" "BHHI" "BHHI")
HEADER_BYTES = _HEADER.size
_FIELDS = ("width", "height", "bit_depth", "frames", "gop", "all_intra", "quality", "imodel_id", "imodel_n", "imodel_m", "imodel_crc",
           "stem_class", "stem_n", "stem_m", "stem_crc")


class FileHeader:
    """the file header as attributes (`_FIELDS`); `pack()` <-> `unpack(bytes)`"""

    def __init__(self, **kw):
        missing = set(_FIELDS) - set(kw)
        if missing or set(kw) - set(_FIELDS):
            raise TypeError(f"FileHeader takes exactly {_FIELDS}, got {sorted(kw)}")
        for k in _FIELDS:
            setattr(self, k, int(kw[k]))

    def astuple(self):
        return tuple(getattr(self, k) for k in _FIELDS)

    def __eq__(self, other):
        return isinstance(other, FileHeader) and self.astuple() == other.astuple()

    def __repr__(self):
        return "FileHeader(" + ", ".join(f"{k}={getattr(self, k)}" for k in _FIELDS) + ")"

    def pack(self):
        self.check()
        return _HEADER.pack(MAGIC, VERSION, *self.astuple())

    @classmethod
    def unpack(cls, data):
        if len(data) < HEADER_BYTES:
            raise ValueError(f"truncated file: the header is {HEADER_BYTES} bytes, got {len(data)}")
        magic, version, *rest = _HEADER.unpack(data[:HEADER_BYTES])
        if magic != MAGIC:
            raise ValueError(f"not a sequence file: magic {magic!r}, expected {MAGIC!r}")
        if version != VERSION:
            raise ValueError(f"sequence file version {version}, this module reads version {VERSION}")
        hdr = cls(**dict(zip(_FIELDS, rest)))
        hdr.check()
        return hdr

    def check(self):
        _check_sides(self.height, self.width)
        if self.bit_depth not in (8, 10):
            raise ValueError(f"bit depth is 8 or 10, got {self.bit_depth}")
        if self.gop < 1 or self.frames < 1:
            raise ValueError(f"a sequence has at least one frame and gop is at least 1, got {self.frames} frames, gop {self.gop}")
        if self.all_intra not in (0, 1):
            raise ValueError(f"the all_intra flag is 0 or 1, got {self.all_intra}")
        if self.imodel_id >= len(bitstream.MODEL_NAMES):
            raise ValueError(f"unknown I-frame model id {self.imodel_id}")
        if self.stem_class != NO_STEM and self.stem_class >= len(STEM_CLASSES):
            raise ValueError(f"unknown STEM class index {self.stem_class}")
        if self.stem_class == NO_STEM and "P" in self.types():
            raise ValueError("the file has P frames and names no STEM class")

    @property
    def imodel_name(self):
        return bitstream.MODEL_NAMES[self.imodel_id]

    def types(self):
        return frame_types(self.frames, self.gop, bool(self.all_intra))


def _check_sides(h, w):
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f"4:2:0 frames have even sides >= 2, got {w} x {h}")


def frame_types(n_frames, gop, all_intra=False):
    """"I" | "P" per frame in display order: evaluation.gop_schedule's rule (frame k, 1-based, with k % gop == 1 is an I frame, and so is the first)"""
    from .evaluation import gop_schedule
    types = [None] * n_frames
    for step in gop_schedule(n_frames, gop, 1, all_intra):
        for index, kind, _ in step:
            types[index] = kind
    return types


def decode_steps(types, concurrent_gops, start=0, stop=None):
    """The order in which the decoder walks the records that frames [start, stop) need (pure).  A GOP that covers part of the range is
    decoded from its I frame up to its last frame inside the range; GOPs outside it are not touched.  Up to `concurrent_gops` of the
    needed GOPs advance together, as in evaluation.gop_schedule, whose steps these are for the whole sequence.
    -> list of steps, each a list of (frame index, "I" | "P", chain)"""
    n = len(types)
    stop = n if stop is None else stop
    if not 0 <= start < stop <= n:
        raise ValueError(f"frames=({start}, {stop}) is no range of a sequence of {n} frames")
    if concurrent_gops < 1:
        raise ValueError(f"concurrent_gops is at least 1, got {concurrent_gops}")
    starts = [i for i, t in enumerate(types) if t == "I"]
    gops = [(c, range(a, min(b, stop))) for c, (a, b) in enumerate(zip(starts, starts[1:] + [n])) if b > start and a < stop]
    steps = []
    for g0 in range(0, len(gops), concurrent_gops):
        group = gops[g0:g0 + concurrent_gops]
        for s in range(max(len(r) for _, r in group)):
            steps.append([(r[s], types[r[s]], chain) for chain, r in group if s < len(r)])
    return steps


def fingerprint(model):
    """zlib.crc32 over the model's state_dict in key order: every key's name, then its tensor's bytes.  The weight of a masked
    convolution is read through its mask (a key "<name>.mask" next to "<name>.weight"): the dead taps never reach a coded symbol, and a
    forward pass zeroes them in place (layers.MaskedConv2d, as in the reference), so a checkpoint saved before the model's first forward
    and one saved after it are the same codec"""
    crc = 0
    sd = model.state_dict()
    for key, value in sd.items():
        crc = zlib.crc32(key.encode(), crc)
        mask = sd.get(key[:-len("weight")] + "mask") if key.endswith(".weight") else None
        if mask is not None:
            value = torch.where(mask != 0, value, torch.zeros_like(value))
        crc = zlib.crc32(value.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes() if value.numel() else b"", crc)
    return crc & 0xFFFFFFFF


def _imodel_classes():
    from . import zoo
    return {"bmshj2018-factorized": zoo.FactorizedPrior, "bmshj2018-hyperprior": zoo.ScaleHyperprior, "mbt2018-mean": zoo.MeanScaleHyperprior,
            "mbt2018": zoo.JointAutoregressiveHierarchicalPriors, "cheng2020-anchor": zoo.Cheng2020Anchor, "cheng2020-attn": zoo.Cheng2020Attention}


def imodel_name(imodel):
    """the zoo name of an I-frame model, by its exact class"""
    for name, cls in _imodel_classes().items():
        if type(imodel) is cls:
            return name
    raise ValueError(f"{type(imodel).__name__} is none of the zoo's I-frame models {bitstream.MODEL_NAMES}")


def _stem_index(stem):
    name = type(stem).__name__
    if name not in STEM_CLASSES:
        raise ValueError(f"{name} is none of the STEM classes {STEM_CLASSES} (the pixel-domain models are not handled here)")
    return STEM_CLASSES.index(name)


def _check_models(imodel, stem, has_p):
    """what can be refused before any device work: -> (I-frame model name, STEM class index or NO_STEM)"""
    name = imodel_name(imodel)
    if not has_p:
        return name, NO_STEM if stem is None else _stem_index(stem)
    if stem is None:
        raise ValueError("the sequence has P frames: a STEM model is needed (or all_intra=True)")
    if not (hasattr(imodel, "getY") and hasattr(imodel, "getX")):
        raise ValueError(f"{name} has no getY / getX: it cannot carry P frames, only all_intra=True sequences")
    index = _stem_index(stem)
    filters = tuple(stem.entropy_bottleneck.filters)
    if filters != (3, 3, 3, 3):
        raise ValueError(f"the STEM model's bottleneck has filters={filters}: the coding engine is built for filters=(3, 3, 3, 3)")
    if int(stem.in_channels) != int(imodel.M):
        raise ValueError(f"the STEM model codes latents of {stem.in_channels} channels, {name} produces {imodel.M}")
    return name, index


def _record_order(model, order):
    """the symbol order of a record coded by `model`: a model without a spatial prior codes in one shot, its records are raster records"""
    return order if getattr(model, "HAS_SPM", False) else "raster"


def _header_for(imodel, stem, h, w, bit_depth, n, gop, all_intra, quality):
    types = frame_types(n, gop, all_intra)
    name, sidx = _check_models(imodel, stem, "P" in types)
    use_stem = sidx != NO_STEM and "P" in types
    return FileHeader(width=w, height=h, bit_depth=bit_depth, frames=n, gop=gop, all_intra=int(bool(all_intra)), quality=quality,
                      imodel_id=bitstream.model_ids[name], imodel_n=imodel.N, imodel_m=imodel.M, imodel_crc=fingerprint(imodel),
                      stem_class=sidx if use_stem else NO_STEM, stem_n=stem.entropy_bottleneck.channels if use_stem else 0,
                      stem_m=stem.in_channels if use_stem else 0, stem_crc=fingerprint(stem) if use_stem else 0)


def check_header(hdr, imodel, stem):
    """ValueError unless the models passed in are the ones the file was written with: class, widths, fingerprint"""
    types = hdr.types()
    name, sidx = _check_models(imodel, stem, "P" in types)
    if name != hdr.imodel_name:
        raise ValueError(f"the file was coded with {hdr.imodel_name}, the I-frame model passed in is {name}")
    if (int(imodel.N), int(imodel.M)) != (hdr.imodel_n, hdr.imodel_m):
        raise ValueError(f"the file's {name} has (N, M) = ({hdr.imodel_n}, {hdr.imodel_m}), the model passed in ({imodel.N}, {imodel.M})")
    if fingerprint(imodel) != hdr.imodel_crc:
        raise ValueError(f"the I-frame model's weights or tables are not the ones the file was coded with (fingerprint {fingerprint(imodel):08x}, "
                         f"file {hdr.imodel_crc:08x})")
    if "P" not in types:
        return
    if sidx != hdr.stem_class:
        raise ValueError(f"the file was coded with {STEM_CLASSES[hdr.stem_class]}, the STEM model passed in is {type(stem).__name__}")
    if (int(stem.entropy_bottleneck.channels), int(stem.in_channels)) != (hdr.stem_n, hdr.stem_m):
        raise ValueError(f"the file's STEM model has (N, M) = ({hdr.stem_n}, {hdr.stem_m}), the model passed in "
                         f"({stem.entropy_bottleneck.channels}, {stem.in_channels})")
    if fingerprint(stem) != hdr.stem_crc:
        raise ValueError(f"the STEM model's weights or tables are not the ones the file was coded with (fingerprint {fingerprint(stem):08x}, "
                         f"file {hdr.stem_crc:08x})")


# ---- records -------------------------------------------------------------------------------------------------------------------
def record_bytes(model_name, quality, order, size, shape, strings):
    """one frame record: bitstream.write_frame's bytes"""
    buf = io.BytesIO()
    bitstream.write_frame(buf, bitstream.get_header(model_name, "mse", quality, order), size, shape, strings)
    return buf.getvalue()


def record_ranges(data, n_frames, offset=HEADER_BYTES):
    """[(first byte, one past the last)] of the `n_frames` records in `data` (the whole file as bytes) from `offset` on, found by the length
    prefixes alone: 2 header bytes, 5 u32 (h, w, shape, the number of strings), then per string a u32 length and that many bytes.
    ValueError when the file ends inside a record or goes on behind the last one."""
    ranges, pos, total = [], offset, len(data)
    for k in range(n_frames):
        first = pos
        if pos + 22 > total:
            raise ValueError(f"truncated file: record {k} starts at byte {pos} of {total} and has no room for its fixed part")
        n_strings = struct.unpack_from(">I", data, pos + 18)[0]
        pos += 22
        for _ in range(n_strings):
            if pos + 4 > total:
                raise ValueError(f"truncated file: record {k} ends inside a string's length at byte {total}")
            pos += 4 + struct.unpack_from(">I", data, pos)[0]
        if pos > total:
            raise ValueError(f"truncated file: record {k} needs bytes up to {pos}, the file has {total}")
        ranges.append((first, pos))
    if pos != total:
        raise ValueError(f"{total - pos} bytes behind the last of {n_frames} records")
    return ranges


def _read_record(data, rng, hdr, index):
    header, size, shape, strings = bitstream.read_frame(io.BytesIO(data[rng[0]:rng[1]]))
    if header[0] != hdr.imodel_name:
        raise ValueError(f"record {index} names the model {header[0]}, the file's header {hdr.imodel_name}")
    if tuple(size) != (hdr.height, hdr.width):
        raise ValueError(f"record {index} holds a frame of {size[1]} x {size[0]}, the file's header says {hdr.width} x {hdr.height}")
    return bitstream.stream_order(header), tuple(shape), strings


# ---- sources -------------------------------------------------------------------------------------------------------------------
class _Source:
    """the frames of encode_sequence: a data.YUVSequence (integer planes through the ingest kernel) or a sequence of [3,h,w] tensors"""

    def __init__(self, frames, device):
        from . import data
        self.device = device
        self.seq = frames if isinstance(frames, data.YUVSequence) else None
        if self.seq is not None:
            self.n, self.h, self.w, self.bit_depth = len(frames), frames.height, frames.width, frames.bit_depth
        else:
            self.frames = frames if hasattr(frames, "__getitem__") and hasattr(frames, "__len__") else list(frames)
            if len(self.frames) == 0:
                raise ValueError("encode_sequence: no frames")
            first = self.frames[0]
            if first.dim() != 3 or first.shape[0] != 3:
                raise ValueError(f"encode_sequence: frames are [3,h,w] tensors, got {tuple(first.shape)}")
            self.n, self.h, self.w = len(self.frames), int(first.shape[1]), int(first.shape[2])
            self.bit_depth = int(getattr(first, "bit_depth", 8))                      # plain tensors: 8 bits, as evaluation._source_planes
        _check_sides(self.h, self.w)

    def padded(self, index):
        """frame `index` as the zero-padded [1,3,Hp,Wp] batch the image model reads (bitstream.pad's centred geometry, multiples of 64)"""
        if self.seq is None:
            x = self.frames[index]
            if tuple(x.shape) != (3, self.h, self.w):
                raise ValueError(f"encode_sequence: frame {index} is {tuple(x.shape)}, the first one [3, {self.h}, {self.w}]")
            return bitstream.pad(x.unsqueeze(0).to(self.device), 64)
        from . import functional as F
        y, u, v = (p.to(self.device, non_blocking=True) for p in self.seq.planes(index))
        return F.yuv420_to_rgb_padded(y, u, v, self.bit_depth, "bilinear", self.seq.clamp, multiple=64)


def _device_of(model):
    return next(model.parameters()).device


def _open(target, mode):
    """(file object, close it afterwards?) of a path or a binary file object"""
    if isinstance(target, (str, os.PathLike)):
        return open(target, mode), True
    return target, False


# ---- the encoder ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def encode_sequence(imodel, stem, frames, out, gop=12, concurrent_gops=8, all_intra=False, order="raster", quality=4):
    """Code `frames` (a data.YUVSequence, or a sequence of [3,h,w] tensors in [0,1] of one size; plain tensors make an 8-bit file) into
    `out` (a path or a binary file object).  Frame types and the walk through the GOPs are evaluation.gop_schedule's; every record holds
    the strings evaluation.eval_gop gives for that frame.  No decoder and no synthesis transform runs: the next frame's condition is the
    encoder's own reconstruction of the latent (`return_y_hat=True`).  stem may be None with all_intra=True.  quality: the 4 bits of the
    records' header the reference's tool fills from its --quality.
    -> {"frames": [{"type", "bytes", "bpp"}] in display order, "bytes": the file's size, "bpp_ave"}"""
    from . import codec, evaluation
    codec._check_order(order)
    src = _Source(frames, _device_of(imodel))
    hdr = _header_for(imodel, stem, src.h, src.w, src.bit_depth, src.n, gop, all_intra, quality)
    name = hdr.imodel_name
    coders = [imodel] + ([stem] if hdr.stem_class != NO_STEM else [])
    if order == "wavefront" and not any(getattr(m, "HAS_SPM", False) for m in coders):
        raise ValueError('order="wavefront": none of the models has a spatial prior -- every record is coded in one shot')
    steps = evaluation.gop_schedule(src.n, gop, concurrent_gops, all_intra)
    fd, close = _open(out, "wb")
    try:
        fd.write(hdr.pack())
        writer = evaluation._InOrder(fd)
        per_frame, y_cond = [None] * src.n, {}
        for step in steps:
            padded = [src.padded(i) for i, _, _ in step]
            ipos = [k for k, (_, kind, _) in enumerate(step) if kind == "I"]
            ppos = [k for k, (_, kind, _) in enumerate(step) if kind == "P"]
            enc, orders = [None] * len(step), [None] * len(step)
            if ipos:
                o = _record_order(imodel, order)
                if getattr(imodel, "HAS_SPM", False):
                    outs = codec.iframe_compress_each(imodel, [padded[k] for k in ipos], order=o, return_y_hat=True)
                else:
                    outs = [imodel.compress(padded[k], return_y_hat=True) for k in ipos]
                for k, e in zip(ipos, outs):
                    enc[k], orders[k] = e, o
            if ppos:
                o = _record_order(stem, order)
                conds = [y_cond[step[k][2]] for k in ppos]
                y_curs = [imodel.getY(padded[k])[0] for k in ppos]
                for k, e in zip(ppos, codec.stem_compress_each(stem, y_curs, conds, order=o, return_y_hat=True)):
                    enc[k], orders[k] = e, o
            for k, (index, kind, _) in enumerate(step):
                rec = record_bytes(name, quality, orders[k], (src.h, src.w), enc[k]["shape"], enc[k]["strings"])
                bits = sum(len(s[0]) for s in enc[k]["strings"]) * 8.0
                per_frame[index] = {"type": kind, "bytes": len(rec), "bpp": bits / (src.h * src.w)}
                writer.put(index, rec)
            y_cond = {chain: enc[k]["y_hat"] for k, (_, _, chain) in enumerate(step)}     # a chain that left the step has ended
    finally:
        if close:
            fd.close()
    return {"frames": per_frame, "bytes": HEADER_BYTES + sum(f["bytes"] for f in per_frame),
            "bpp_ave": sum(f["bpp"] for f in per_frame) / len(per_frame)}


# ---- the decoder ---------------------------------------------------------------------------------------------------------------
def _planes_bytes(planes):
    from . import data
    buf = io.BytesIO()
    data._write_planes(buf, planes, append=True)
    return buf.getvalue()


@torch.no_grad()
def decode_sequence(imodel, stem, src, write_to=None, concurrent_gops=8, frames=None, return_frames=True):
    """Decode the file `src` (a path, bytes, or a binary file object) with nothing else: its header is checked against the two models
    (`check_header`), then every GOP is rebuilt from its records -- I frames by the image model's decompress, P frames by the STEM model's
    given the previous frame's decoded latent, pixels by getX -- with up to `concurrent_gops` GOPs side by side.  write_to (a path or a
    binary file object) receives the frames in display order as raw planar 4:2:0 at the file's bit depth, quantised from the padded
    x_hat by one kernel per frame (functional.rgb_window_to_yuv420).  frames=(start, stop): only those frames are emitted, and only the
    GOPs that cover them are decoded; the other records are stepped over.
    -> the cropped x_hat tensors [1,3,h,w] of the emitted frames in display order (an empty list with return_frames=False)"""
    from . import codec, evaluation
    from . import functional as F
    if isinstance(src, (bytes, bytearray, memoryview)):
        data = bytes(src)
    else:
        fd, close = _open(src, "rb")
        try:
            data = fd.read()
        finally:
            if close:
                fd.close()
    hdr = FileHeader.unpack(data)
    check_header(hdr, imodel, stem)
    ranges = record_ranges(data, hdr.frames)
    types = hdr.types()
    start, stop = (0, hdr.frames) if frames is None else (int(frames[0]), int(frames[1]))
    steps = decode_steps(types, concurrent_gops, start, stop)
    h, w = hdr.height, hdr.width
    sink, close = _open(write_to, "wb") if write_to is not None else (None, False)
    try:
        writer = evaluation._InOrder(sink) if sink is not None else None
        kept, y_cond = [None] * (stop - start), {}
        for step in steps:
            recs = [_read_record(data, ranges[i], hdr, i) for i, _, _ in step]
            y_hat, x_hat = [None] * len(step), [None] * len(step)
            for kind in ("I", "P"):
                pos = [k for k, (_, t, _) in enumerate(step) if t == kind]
                if not pos:
                    continue
                orders = {recs[k][0] for k in pos}
                if len(orders) != 1:
                    raise ValueError(f"the {kind} records of frames {[step[k][0] for k in pos]} mix symbol orders")
                o = orders.pop()
                strings, shapes = [recs[k][2] for k in pos], [recs[k][1] for k in pos]
                if kind == "I" and getattr(imodel, "HAS_SPM", False):
                    outs = codec.iframe_decompress_each(imodel, strings, shapes, order=o)
                elif kind == "I":
                    if o != "raster":
                        raise ValueError(f"{hdr.imodel_name} codes in one shot: its records cannot be in wavefront order")
                    outs = [imodel.decompress(s, sh) for s, sh in zip(strings, shapes)]
                else:
                    ys = codec.stem_decompress_each(stem, strings, shapes, [y_cond[step[k][2]] for k in pos], order=o)
                    outs = [{"y_hat": y, "x_hat": imodel.getX(y)} for y in ys]
                for k, d in zip(pos, outs):
                    y_hat[k], x_hat[k] = d["y_hat"], d["x_hat"]
            for k, (index, _, _) in enumerate(step):
                if index < start:
                    continue                                                          # decoded for the chain's sake only
                if writer is not None:
                    writer.put(index - start, _planes_bytes(F.rgb_window_to_yuv420(x_hat[k], (h, w), hdr.bit_depth)))
                if return_frames:
                    kept[index - start] = bitstream.crop(x_hat[k], (h, w))
            y_cond = {chain: y_hat[k] for k, (_, _, chain) in enumerate(step)}
    finally:
        if close:
            sink.close()
    return kept if return_frames else []


# ---- the command line ----------------------------------------------------------------------------------------------------------
def _state_dict(path):
    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd and not any(torch.is_tensor(v) for v in sd.values()):
        sd = sd["state_dict"]
    if not isinstance(sd, dict) or not sd or not all(torch.is_tensor(v) for v in sd.values()):
        raise ValueError(f"{path} holds no state_dict")
    return sd


def load_imodel(name, path, device):
    """an I-frame model of the zoo sized by, and loaded from, the checkpoint at `path` (a state_dict, tables included)"""
    classes = _imodel_classes()
    if name not in classes:
        raise ValueError(f'unknown I-frame model "{name}": one of {tuple(classes)}')
    try:
        return classes[name].from_state_dict(_state_dict(path)).to(device).eval()
    except (KeyError, RuntimeError) as e:
        raise ValueError(f"{path} is no checkpoint of {name}: {e}") from e


def load_stem(cls_name, path, device):
    """a STEM model of class `cls_name` sized by, and loaded from, the checkpoint at `path`"""
    from . import models
    if cls_name not in STEM_CLASSES:
        raise ValueError(f'unknown STEM class "{cls_name}": one of {STEM_CLASSES}')
    sd = _state_dict(path)
    try:
        net = getattr(models, cls_name)(sd["entropy_bottleneck.quantiles"].size(0), sd["HD.4.weight"].size(0) // 2)
        net.load_state_dict(sd)
    except (KeyError, RuntimeError) as e:
        raise ValueError(f"{path} is no checkpoint of {cls_name}: {e}") from e
    return net.to(device).eval()


def _parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m spatiotemporalentropymodel_amd.video", description="stand-alone sequence codec")
    sub = p.add_subparsers(dest="command", required=True)
    for name in ("encode", "decode"):
        s = sub.add_parser(name)
        s.add_argument("--imodel", required=True, help="zoo name of the I-frame model")
        s.add_argument("--imodel-checkpoint", required=True)
        s.add_argument("--stem", default=None, help="STEM class name (not needed for an all-intra file)")
        s.add_argument("--stem-checkpoint", default=None)
        s.add_argument("--input", required=True)
        s.add_argument("--output", required=True)
        s.add_argument("--concurrent-gops", type=int, default=8)
        s.add_argument("--device", default="cuda:0")
    e, d = sub.choices["encode"], sub.choices["decode"]
    e.add_argument("--width", type=int, required=True)
    e.add_argument("--height", type=int, required=True)
    e.add_argument("--bit-depth", type=int, default=8)
    e.add_argument("--frames", type=int, default=None, help="code the first so many frames")
    e.add_argument("--gop", type=int, default=12)
    e.add_argument("--all-intra", action="store_true")
    e.add_argument("--order", default="raster", choices=("raster", "wavefront"))
    e.add_argument("--quality", type=int, default=4)
    d.add_argument("--frames", default=None, help="START:STOP, decode only these frames")
    return p


def main(argv=None):
    """-> the exit status: 0, or 2 after a refusal (ValueError), whose message goes to stderr"""
    args = _parser().parse_args(argv)
    try:
        if (args.stem is None) != (args.stem_checkpoint is None):
            raise ValueError("--stem and --stem-checkpoint come together")
        imodel = load_imodel(args.imodel, args.imodel_checkpoint, args.device)
        stem = load_stem(args.stem, args.stem_checkpoint, args.device) if args.stem else None
        if args.command == "encode":
            from . import data
            seq = data.YUVSequence(args.input, args.width, args.height, args.bit_depth, frames=args.frames, device=args.device)
            res = encode_sequence(imodel, stem, seq, args.output, gop=args.gop, concurrent_gops=args.concurrent_gops, all_intra=args.all_intra,
                                  order=args.order, quality=args.quality)
            print(f"{len(res['frames'])} frames, {res['bytes']} bytes, {res['bpp_ave']:.6f} bpp")
        else:
            rng = None
            if args.frames is not None:
                try:
                    rng = tuple(int(v) for v in args.frames.split(":"))
                    assert len(rng) == 2
                except (ValueError, AssertionError):
                    raise ValueError(f"--frames is START:STOP, got {args.frames!r}") from None
            decode_sequence(imodel, stem, args.input, write_to=args.output, concurrent_gops=args.concurrent_gops, frames=rng, return_frames=False)
            print(f"decoded {args.input} into {args.output}")
    except ValueError as e:
        print(f"refused: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
