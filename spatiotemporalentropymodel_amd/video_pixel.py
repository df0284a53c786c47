"""The stand-alone sequence codec of the PIXEL-domain model pairs -- stem_roi_i + stem_roi driven by a quality map (the reference's
variable-rate / region-of-interest codec), and an image model of the zoo + one of the fixed-rate pixel models.  video.py is the same
thing for the latent-domain STEM pairs; both are formats of seqfile.py's container.

    encode_sequence(model_i, model_p, frames, out, qmaps=... | rois=..., ...)    frames (+ maps or rectangles) -> file; no decompress
    decode_sequence(model_i, model_p, src, write_to=None, ...)                   file -> planar 4:2:0 frames (and the cropped x_hat)
    verify_sequence(model_i, model_p, src)                                       file -> a report: every frame's state hash checked
    python -m spatiotemporalentropymodel_amd.video_pixel encode|decode|verify ...

evaluation.eval_gop_pixel compresses and decompresses every frame with the same objects, takes its quality maps as host tensors and
crops and re-pads the reconstruction with eager torch between frames.  Here a frame costs the encoder one compress: the reconstruction
the next P frame is conditioned on comes from the encoder's own symbols (`return_x_hat=True` of the pixel models, `return_y_hat=True`
+ getX of a zoo model), and one kernel turns that padded frame into the condition IN PLACE (functional.rgb_window_recondition: the
reference conditions on the CROPPED reconstruction, zero-padded again, so the border must become zero).  In the decoder the same
kernel, in the same pass, also writes the frame's integer 4:2:0 planes.  Rectangles are rasterised on the device straight into the
padded map a model reads (functional.roi_map_padded).  Every record holds the strings and the shape eval_gop_pixel gives for that
frame with the same maps.

`concurrent_gops` is deliberately not offered: these models code a frame in one shot and their transforms must run at batch 1 (README,
"Why the transforms stay at batch 1"), so there is nothing to batch across GOPs.

File layout (seqfile.py's container -- frame types, record ranges, the state-hash trailer, the fingerprint and the order of checks are
stated there -- with this header and this record rule; all integers big-endian):

    header   4s magic "STPX" | u8 version | u32 w | u32 h | u8 bit depth | u32 frames | u32 gop | u8 all_intra | u8 quality
             | u8 I kind (0..5: bitstream.model_ids, a, b = N, M; 64: stem_roi_i, a, b = bottleneck channels, in_channels) | u16 a | u16 b
             | u32 fingerprint
             | u8 P kind (index in PIXEL_P_CLASSES; 255: none, an all-intra file) | u16 a | u16 b | u32 fingerprint
    records  one per frame in display order, in bitstream.write_frame's layout

A record's first byte is the I kind for an I record and 128 + the P kind for a P record; its second byte is (quality - 1) & 0x0F.  For
an I-frame model of the zoo an I record therefore is byte for byte the record the reference's tool writes for that image.  The quality
map is not in the file: it is encoder-side information, the decoder derives its modulation from z_hat (PDecoder).

The hashed state of a frame (seqfile.py, "State hashes") is its padded x_hat AFTER functional.rgb_window_recondition -- the whole padded
tensor with its border zeroed, exactly the next P frame's condition.  Here the state is a picture, so checking it needs the synthesis:
verify_sequence runs the whole decoder and only leaves out the planes and the file.
"""
from __future__ import annotations

import io
import struct
import sys

import torch

from . import bitstream, seqfile
from .seqfile import (HEADER_BYTES, STATE_HASH_BIT, VERSION, _HEADER, StateMismatch, _open, _planes_bytes, _Source,  # noqa: F401  (this module's names too)
                      decode_steps, fingerprint, frame_types, gop_starts, hashed_record_ranges, print_report, record_ranges, split_trailer,
                      trailer_bytes)

#: the P-frame model's index in the file header
PIXEL_P_CLASSES = ("stem_baseline", "stem_baselinev2", "stem_roi", "stem_roi_wo_gsc")
NO_P = 255
#: the I kind of stem_roi_i; 0..5 are bitstream.model_ids
KIND_ROI_I = 64
#: added to the P kind in a P record's first byte
P_RECORD = 128


class FileHeader(seqfile.FileHeader):
    """seqfile.FileHeader under the magic "STPX": either model by its kind and two widths (a, b)"""
    MAGIC = b"STPX"
    FIELDS = seqfile.COMMON_FIELDS + ("i_kind", "i_a", "i_b", "i_crc", "p_kind", "p_a", "p_b", "p_crc")
    NOUN = "pixel-domain sequence file"
    FOREIGN = {b"STMV": "this is a file of the latent-domain codec (magic b'STMV'): read it with spatiotemporalentropymodel_amd.video"}

    def check_models(self):
        if self.i_kind != KIND_ROI_I and self.i_kind >= len(bitstream.MODEL_NAMES):
            raise ValueError(f"unknown I kind {self.i_kind}")
        if self.p_kind != NO_P and self.p_kind >= len(PIXEL_P_CLASSES):
            raise ValueError(f"unknown P kind {self.p_kind}")
        if self.p_kind == NO_P and "P" in self.types():
            raise ValueError("the file has P frames and names no P-frame class")

    @property
    def i_name(self):
        return "stem_roi_i" if self.i_kind == KIND_ROI_I else bitstream.MODEL_NAMES[self.i_kind]

    def record_byte(self, kind):
        """the first byte of an "I" | "P" record of this file"""
        return self.i_kind if kind == "I" else P_RECORD + self.p_kind


MAGIC, _FIELDS = FileHeader.MAGIC, FileHeader.FIELDS


def read_state_hashes(data):
    """seqfile.read_state_hashes for this module's files: the state hashes in display order, or None for an un-hashed file"""
    return seqfile.read_state_hashes(data, FileHeader)


# ---- models --------------------------------------------------------------------------------------------------------------------
def _i_kind(model_i):
    """-> (I kind, a, b), or ValueError: stem_roi_i, or a zoo model that can reconstruct from its own symbols (getX)"""
    from . import video
    if type(model_i).__name__ == "stem_roi_i":
        return KIND_ROI_I, int(model_i.entropy_bottleneck.channels), int(model_i.in_channels)
    if type(model_i).__name__ in PIXEL_P_CLASSES:
        raise ValueError(f"{type(model_i).__name__} is a P-frame model: the I-frame model is stem_roi_i or one of {bitstream.MODEL_NAMES}")
    name = video.imodel_name(model_i)
    if not hasattr(model_i, "getX"):
        raise ValueError(f"{name} has no getX: this codec needs the reconstruction from the encoder's own symbols; code its latents with "
                         "video.encode_sequence instead")
    return bitstream.model_ids[name], int(model_i.N), int(model_i.M)


def _p_kind(model_p):
    name = type(model_p).__name__
    if name not in PIXEL_P_CLASSES:
        raise ValueError(f"{name} is none of the pixel-domain P-frame classes {PIXEL_P_CLASSES}")
    return PIXEL_P_CLASSES.index(name), int(model_p.entropy_bottleneck.channels), int(model_p.in_channels)


def _check_models(model_i, model_p, has_p):
    """what can be refused before any device work: -> ((I kind, a, b), (P kind, a, b) or None)"""
    i = _i_kind(model_i)
    if not has_p:
        return i, None
    if model_p is None:
        raise ValueError("the sequence has P frames: a P-frame model is needed (or all_intra=True)")
    return i, _p_kind(model_p)


def _takes_qmap(model):
    return bool(getattr(model, "QMAP", False))


def _header_for(model_i, model_p, h, w, bit_depth, n, gop, all_intra, quality, state_hash=False):
    types = frame_types(n, gop, all_intra)
    (ik, ia, ib), p = _check_models(model_i, model_p, "P" in types)
    pk, pa, pb = p if p is not None else (NO_P, 0, 0)
    return FileHeader(state_hash=state_hash, width=w, height=h, bit_depth=bit_depth, frames=n, gop=gop, all_intra=int(bool(all_intra)),
                      quality=quality, i_kind=ik, i_a=ia, i_b=ib, i_crc=fingerprint(model_i), p_kind=pk, p_a=pa, p_b=pb,
                      p_crc=fingerprint(model_p) if p is not None else 0)


def check_header(hdr, model_i, model_p):
    """ValueError unless the models passed in are the ones the file was written with: class, widths, fingerprint.  A kind is the kind
    byte of the header; the widths are its (a, b)."""
    (ik, ia, ib), p = _check_models(model_i, model_p, "P" in hdr.types())
    seqfile.check_side("I-frame", model_i, (hdr.i_kind, hdr.i_name, (hdr.i_a, hdr.i_b), hdr.i_crc), (ik, type(model_i).__name__, (ia, ib)), hdr.i_name)
    if p is not None:
        p_name = PIXEL_P_CLASSES[hdr.p_kind]
        seqfile.check_side("P-frame", model_p, (hdr.p_kind, p_name, (hdr.p_a, hdr.p_b), hdr.p_crc), (p[0], type(model_p).__name__, p[1:]), p_name)


# ---- records -------------------------------------------------------------------------------------------------------------------
def record_bytes(first_byte, quality, size, shape, strings):
    """one frame record: bitstream.write_frame's bytes under this module's two header bytes"""
    buf = io.BytesIO()
    bitstream.write_frame(buf, (first_byte, (quality - 1) & 0x0F), size, shape, strings)
    return buf.getvalue()


def read_record(data, rng, hdr, index, kind):
    """the record of frame `index` (an "I" | "P" frame by the header) at data[rng[0]:rng[1]] -> (shape, strings); ValueError when its
    first byte or its frame size contradicts the header"""
    pos = rng[0]
    first, _, h, w, s0, s1, n_strings = struct.unpack_from(">BBIIIII", data, pos)
    if first != hdr.record_byte(kind):
        raise ValueError(f"record {index} starts with byte {first}, frame {index} is an {kind} frame of this file: byte {hdr.record_byte(kind)}")
    if (h, w) != (hdr.height, hdr.width):
        raise ValueError(f"record {index} holds a frame of {w} x {h}, the file's header says {hdr.width} x {hdr.height}")
    pos += 22
    strings = []
    for _ in range(n_strings):
        n = struct.unpack_from(">I", data, pos)[0]
        strings.append([bytes(data[pos + 4:pos + 4 + n])])
        pos += 4 + n
    return (s0, s1), strings


# ---- maps ----------------------------------------------------------------------------------------------------------------------
def _map_source(qmaps, rois, level, h, w, device):
    """-> a function index -> the padded quality map [1,1,Hp,Wp] on the device, or None; to be called once per frame, in order.
    At most one of qmaps and rois is given (encode_sequence has refused both)."""
    from . import evaluation
    from . import functional as F
    if rois is not None:
        boxes_of = rois if callable(rois) else None
        if boxes_of is None:
            rois = list(rois)

        def rasterised(index):
            if boxes_of is None and index >= len(rois):
                raise ValueError(f"rois ran out at frame {index}: a list of box lists is parallel to the frames")
            return F.roi_map_padded(boxes_of(index) if boxes_of is not None else rois[index], (h, w), background=level, device=device)

        return rasterised
    if qmaps is None:
        return lambda index: None
    map_of = evaluation._per_frame_maps(qmaps)

    def padded(index):
        q = map_of(index, h, w)
        return None if q is None else bitstream.pad(evaluation.quality_map(q, h, w).to(device), 64)

    return padded


# ---- the encoder ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def encode_sequence(model_i, model_p, frames, out, *, qmaps=None, rois=None, level=0.0, gop=12, all_intra=False, quality=4, state_hash=False):
    """Code `frames` (a data.YUVSequence, or a sequence of [3,h,w] tensors in [0,1] of one size; plain tensors make an 8-bit file) into
    `out` (a path or a binary file object).  Frame types are evaluation.eval_gop_pixel's; every record holds the strings and the shape
    it gives for that frame with the same maps.  qmaps: its four forms (None; one map for every frame; an iterable parallel to the
    frames; a callable (index, h, w) -> map), each map through evaluation.quality_map.  rois: instead, a list of boxes
    (x0, y0, x1, y1, value[, feather]) for every frame, or a callable index -> such a list, rasterised on the device over the
    background `level` (functional.roi_map_padded).  A map goes only to the models that take one (QMAP).  Per frame: one compress with
    the reconstruction from the encoder's own symbols, one kernel that makes it the next condition in place, one record; no decompress.
    model_p may be None with all_intra=True.  state_hash=True: a hashed file -- bit 7 of the version byte and, behind the last record,
    every frame's functional.state_hash of the reconditioned padded x_hat (the next condition); the hashes collect in one device buffer
    that one copy fetches at the end.  The records are those of the un-hashed file.
    -> {"frames": [{"type", "bytes", "bpp"}] in display order, "bytes": the file's size, "bpp_ave"} and, with state_hash, "state_hash":
    the hashes in display order"""
    from . import functional as F
    device = seqfile._device_of(model_i)
    src = _Source(frames, device)
    hdr = _header_for(model_i, model_p, src.h, src.w, src.bit_depth, src.n, gop, all_intra, quality, state_hash)
    types = hdr.types()
    coders = [model_i] + ([model_p] if "P" in types else [])
    if qmaps is not None and rois is not None:
        raise ValueError("qmaps and rois are mutually exclusive: give the maps or the rectangles")
    given = qmaps is not None or rois is not None
    if given and not any(_takes_qmap(m) for m in coders):
        raise ValueError(f"a quality map is given and none of the coding models takes one ({', '.join(type(m).__name__ for m in coders)})")
    if not given:
        for m in coders:
            if _takes_qmap(m):
                raise ValueError(f"{type(m).__name__} takes a quality map: give qmaps= or rois=")
    map_of = _map_source(qmaps, rois, level, src.h, src.w, device)
    h, w = src.h, src.w
    fd, close = _open(out, "wb")
    try:
        fd.write(hdr.pack())
        per_frame, x_cond = [], None
        hbuf = torch.empty(src.n, dtype=torch.int64, device=device) if state_hash else None
        for index, kind in enumerate(types):
            model = model_i if kind == "I" else model_p
            x = src.padded(index)
            q = map_of(index)
            ins = [x] + ([x_cond] if kind == "P" else [])
            if _takes_qmap(model):
                if q is None:
                    raise ValueError(f"{type(model).__name__} takes a quality map and frame {index} has none")
                ins.append(q)
            if kind == "I" and hdr.i_kind != KIND_ROI_I:
                enc = model.compress(x, return_y_hat=True)
                x_hat = model.getX(enc["y_hat"])
            else:
                enc = model.compress(*ins, return_x_hat=True)
                x_hat = enc["x_hat"]
            F.rgb_window_recondition(x_hat, (h, w))
            x_cond = x_hat
            if state_hash:
                F.state_hash(x_hat, out=hbuf[index:index + 1])
            rec = record_bytes(hdr.record_byte(kind), quality, (h, w), enc["shape"], enc["strings"])
            fd.write(rec)
            bits = sum(len(s[0]) for s in enc["strings"]) * 8.0
            per_frame.append({"type": kind, "bytes": len(rec), "bpp": bits / (h * w)})
        hashes = F.state_hash_ints(hbuf) if state_hash else None
        if state_hash:
            fd.write(trailer_bytes(hashes))
    finally:
        if close:
            fd.close()
    res = {"frames": per_frame, "bytes": HEADER_BYTES + sum(f["bytes"] for f in per_frame) + (8 * src.n if state_hash else 0),
           "bpp_ave": sum(f["bpp"] for f in per_frame) / len(per_frame)}
    if state_hash:
        res["state_hash"] = hashes
    return res


# ---- the decoder ---------------------------------------------------------------------------------------------------------------
def _walk(model_i, model_p, hdr, data, ranges, steps, hashed, planes_from=None, abandoned=lambda index: False):
    """The decoder's walk over `steps` (decode_steps at one GOP at a time): per frame, its record is read and decoded -- I frames by
    model_i's decompress, P frames by model_p's given the previous frame's state --, one kernel (functional.rgb_window_recondition)
    makes the padded x_hat the next condition in place and, for the frames from `planes_from` on (None: for none), writes its integer
    4:2:0 planes in the same pass, and, when `hashed`, the state is hashed and fetched -> yields (index, kind, (x_hat, planes or None),
    hash or None) BEFORE the state becomes a condition.  Frames for which abandoned(index) holds when their turn comes are left out."""
    from . import functional as F
    x_cond = None
    for (index, kind, _), in steps:
        if abandoned(index):
            continue
        shape, strings = read_record(data, ranges[index], hdr, index, kind)
        if kind == "I":
            x_hat = model_i.decompress(strings, shape)["x_hat"]
        else:
            x_hat = model_p.decompress(strings, shape, x_cond)["x_hat"]
        emit = planes_from is not None and index >= planes_from
        planes = F.rgb_window_recondition(x_hat, (hdr.height, hdr.width), hdr.bit_depth if emit else None)
        yield index, kind, (x_hat, planes), F.state_hash_ints(F.state_hash(x_hat))[0] if hashed else None
        x_cond = x_hat


@torch.no_grad()
def decode_sequence(model_i, model_p, src, write_to=None, frames=None, return_frames=True, verify=True):
    """Decode the file `src` (a path, bytes, or a binary file object) with nothing but the file and the two models: the quality map is
    encoder-side information and is not needed -- the decoder derives its modulation from z_hat (PDecoder).  The file is checked, then
    its header against the models (seqfile.open_for_decoding, `check_header`: kind, widths, fingerprint), then every GOP is rebuilt from
    its records: I frames by model_i's decompress, P frames by model_p's given the previous frame's reconstruction.  One kernel per frame
    (functional.rgb_window_recondition) makes the decoded padded frame the next condition in place and, when write_to (a path or a
    binary file object) is given, writes the frame's planar 4:2:0 samples at the file's bit depth in the same pass.
    frames=(start, stop): only those frames are emitted, and only the GOPs that cover them are decoded.  On a hashed file
    (encode_sequence(state_hash=True)) with verify=True every decoded frame's reconditioned x_hat -- also of frames decoded for the
    chain's sake only -- is hashed and compared with the file's entry before it becomes a condition or leaves as a picture:
    StateMismatch at the first difference.  verify=False, or an un-hashed file: nothing is hashed.
    -> the cropped x_hat tensors [1,3,h,w] of the emitted frames in display order, as copies (an empty list with return_frames=False)"""
    hdr, data, ranges, want, types, starts = seqfile.open_for_decoding(src, FileHeader, lambda hdr: check_header(hdr, model_i, model_p))
    start, stop = (0, hdr.frames) if frames is None else (int(frames[0]), int(frames[1]))
    steps = decode_steps(types, 1, start, stop)
    h, w = hdr.height, hdr.width
    sink, close = _open(write_to, "wb") if write_to is not None else (None, False)
    try:
        kept = []
        for index, _, (x_hat, planes), got in _walk(model_i, model_p, hdr, data, ranges, steps, verify and want is not None,
                                                    planes_from=start if sink is not None else None):
            if got is not None and got != want[index]:
                raise StateMismatch(index, starts[index], want[index], got)
            if planes is not None:
                sink.write(_planes_bytes(planes))
            if index >= start and return_frames:                                      # otherwise decoded for the chain's sake only
                top, left = (x_hat.size(2) - h) // 2, (x_hat.size(3) - w) // 2
                kept.append(x_hat[:, :, top:top + h, left:left + w].clone())
    finally:
        if close:
            sink.close()
    return kept


@torch.no_grad()
def verify_sequence(model_i, model_p, src):
    """Check a hashed file against this decoder: every GOP is decoded on its own (the state is a picture, so the synthesis runs; no
    planes, no file) and every frame's reconditioned x_hat is hashed and compared with the file's entry.  A GOP is abandoned at its
    first mismatch -- what follows would be decoded under a wrong condition -- and the next GOP goes on.
    -> video.verify_sequence's report (seqfile.VerifyReport).  ValueError for an un-hashed file."""
    hdr, data, ranges, want, types, starts = seqfile.open_for_decoding(src, FileHeader, lambda hdr: check_header(hdr, model_i, model_p), need_hashes=True)
    report = seqfile.VerifyReport(hdr, starts, want)
    for index, _, _, got in _walk(model_i, model_p, hdr, data, ranges, decode_steps(types, 1), True, abandoned=report.abandoned):
        report.check(index, got)
    return report.result()


# ---- the command line ----------------------------------------------------------------------------------------------------------
def load_model_i(name, path, device):
    """stem_roi_i, or an I-frame model of the zoo, sized by and loaded from the checkpoint at `path`"""
    from . import video
    return _load_pixel(name, path, device) if name == "stem_roi_i" else video.load_imodel(name, path, device)


def _load_pixel(cls_name, path, device):
    return seqfile.load_sized(cls_name, path, device, "entropy_bottleneck.quantiles", "EPM.4.weight")


def load_model_p(cls_name, path, device):
    """a pixel-domain P-frame model of class `cls_name`, sized by and loaded from the checkpoint at `path`"""
    if cls_name not in PIXEL_P_CLASSES:
        raise ValueError(f'unknown P-frame class "{cls_name}": one of {PIXEL_P_CLASSES}')
    return _load_pixel(cls_name, path, device)


def parse_roi(text):
    """--roi x0,y0,x1,y1,value[,feather] -> the box tuple"""
    parts = text.split(",")
    try:
        if len(parts) not in (5, 6):
            raise ValueError
        box = tuple(int(p) for p in parts[:4]) + (float(parts[4]),)
        return box + ((int(parts[5]),) if len(parts) == 6 else ())
    except ValueError:
        raise ValueError(f"--roi is x0,y0,x1,y1,value[,feather], got {text!r}") from None


def parse_roi_file(lines):
    """lines `frame x0 y0 x1 y1 value [feather]`; `#` starts a comment -> {frame index: [box, ...]} in the file's order"""
    per_frame = {}
    for number, line in enumerate(lines, start=1):
        fields = line.split("#", 1)[0].split()
        if not fields:
            continue
        try:
            if len(fields) not in (6, 7):
                raise ValueError
            frame = int(fields[0])
            box = tuple(int(p) for p in fields[1:5]) + (float(fields[5]),) + ((int(fields[6]),) if len(fields) == 7 else ())
            if frame < 0:
                raise ValueError
        except ValueError:
            raise ValueError(f"--roi-file line {number} is `frame x0 y0 x1 y1 value [feather]`, got {line.strip()!r}") from None
        per_frame.setdefault(frame, []).append(box)
    return per_frame


def _parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m spatiotemporalentropymodel_amd.video_pixel", description="stand-alone pixel-domain sequence codec")
    subs = seqfile.add_common_options(p.add_subparsers(dest="command", required=True), "model-i", "stem_roi_i, or the zoo name of an I-frame model",
                                      "model-p", f"one of {PIXEL_P_CLASSES} (not needed for an all-intra file)")
    seqfile.add_coding_options(subs["encode"], subs["decode"])
    e = subs["encode"]
    e.add_argument("--level", type=float, default=None, help="the quality level outside every rectangle, in [0, 1]")
    e.add_argument("--roi", action="append", default=[], help="x0,y0,x1,y1,value[,feather]: a rectangle of every frame (repeatable)")
    e.add_argument("--roi-file", default=None, help="lines `frame x0 y0 x1 y1 value [feather]`; # starts a comment")
    return p


def _cli_rois(args):
    """the rois= argument of the command line: None when neither a level nor a rectangle is given"""
    every = [parse_roi(t) for t in args.roi]
    per_frame = {}
    if args.roi_file is not None:
        with open(args.roi_file) as f:
            per_frame = parse_roi_file(f)
    if args.level is None and not every and not per_frame:
        return None
    return lambda index: every + per_frame.get(index, [])


def _run(args):
    if (args.model_p is None) != (args.model_p_checkpoint is None):
        raise ValueError("--model-p and --model-p-checkpoint come together")
    rois = _cli_rois(args) if args.command == "encode" else None
    model_i = load_model_i(args.model_i, args.model_i_checkpoint, args.device)
    model_p = load_model_p(args.model_p, args.model_p_checkpoint, args.device) if args.model_p else None
    return seqfile.run_command(
        args,
        encode=lambda seq: encode_sequence(model_i, model_p, seq, args.output, rois=rois, level=args.level if args.level is not None else 0.0,
                                           gop=args.gop, all_intra=args.all_intra, quality=args.quality, state_hash=args.state_hash),
        decode=lambda rng: decode_sequence(model_i, model_p, args.input, write_to=args.output, frames=rng, return_frames=False,
                                           verify=not args.no_verify),
        verify=lambda: verify_sequence(model_i, model_p, args.input))


def main(argv=None):
    """-> the exit status: 0; 2 after a refusal (ValueError), whose message goes to stderr; 3 when a state hash did not match (`verify`
    prints its report as JSON either way, `decode` stops at the first one)"""
    return seqfile.exit_status(_run, _parser().parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
