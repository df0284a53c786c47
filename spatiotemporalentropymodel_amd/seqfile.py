"""The container of the two stand-alone sequence codecs: what belongs to the FILE and not to a model family.  video.py (latent-domain
STEM pairs, magic "STMV") and video_pixel.py (pixel-domain pairs, magic "STPX") subclass the header, say what a model "kind" is, and
code the records; everything else about the file is stated here, once.

A file is a 42-byte header (magic, version, geometry, frames, gop, and per model a kind, two widths and a fingerprint: the two modules'
docstrings have the tables), one record per frame in display order in bitstream.write_frame's layout and, in a hashed file, a trailer.
All integers are big-endian, as in bitstream.py.  Frame k is an I or a P frame by its index and `gop` (evaluation.gop_schedule's rule),
so a record needs no type field.  A record is skipped without parsing its strings, by the length prefixes (`record_ranges`): decoding
frames=(start, stop) touches only the GOPs that cover the range (`decode_steps`).

State hashes (opt-in: encode_sequence(state_hash=True), `encode --state-hash`).  Both codecs are closed-loop: frame t is decoded under
priors computed from the decoder's own state of frame t - 1, so a decoder whose arithmetic differs in one last bit -- another tile plan,
another build of the library -- decodes plausible garbage from there to the end of the GOP.  A hashed file carries bit 7 in its version
byte (STATE_HASH_BIT, in the manner of bitstream.ORDER_BIT) and, behind the last record, a trailer of `frames` u64: per frame in display
order, functional.state_hash of the state the next P frame is conditioned on, from the encoder's own reconstruction.  Header and records
are byte for byte the un-hashed file's but for that bit; the trailer sits 8 * frames bytes from the end, so a partial decode finds its
entries without parsing further.  A decoder compares every decoded frame's hash BEFORE the state becomes a condition and raises
StateMismatch; verify_sequence checks a whole file and reports (`VerifyReport`).

The fingerprint is zlib.crc32 over a model's state_dict in key order: each key's name, then the tensor's bytes (a masked convolution's
weight through its mask: `fingerprint`).  It covers the weights and the integer CDF tables (buffers of the entropy models): a decoder
with other weights, or with tables rebuilt on another host's libm, would decode garbage without noticing, so it refuses instead.  It is
a check against mistakes, not against tampering.

The order of checks when a file is opened for decoding (`open_for_decoding`, used by decode_sequence and verify_sequence of both
codecs): the file's own consistency first -- header, records, trailer: it costs nothing -- then the models against the header -- class,
widths, fingerprint: the fingerprint reads every weight -- and last, for verify_sequence, the refusal of an un-hashed file.  When both
the file and the models are wrong, the file's error is the one reported.
"""
from __future__ import annotations

import io
import os
import struct
import sys
import zlib

import torch

from . import bitstream

VERSION = 1
#: bit 7 of the version byte: behind the last record the file has a trailer of one u64 state hash per frame
STATE_HASH_BIT = 0x80
_HEADER = struct.Struct(">4sBIIBIIBB" "BHHI" "BHHI")
HEADER_BYTES = _HEADER.size
COMMON_FIELDS = ("width", "height", "bit_depth", "frames", "gop", "all_intra", "quality")


class FileHeader:
    """the file header as attributes (`FIELDS`); `pack()` <-> `unpack(bytes)`.  `state_hash` (outside `FIELDS`: it is a bit of the
    version byte, not a field of the struct) says that the file ends in a trailer of state hashes.  A format subclasses this with its
    MAGIC, its FIELDS (COMMON_FIELDS + the names of its eight model fields) and `check_models`; NOUN is what its refusals call the
    file, FOREIGN maps another format's magic to the refusal that names its reader."""
    MAGIC = None
    FIELDS = COMMON_FIELDS
    NOUN = "sequence file"
    FOREIGN = {}

    def __init__(self, state_hash=False, **kw):
        if set(kw) != set(self.FIELDS):
            raise TypeError(f"FileHeader takes exactly {self.FIELDS}, got {sorted(kw)}")
        for k in self.FIELDS:
            setattr(self, k, int(kw[k]))
        self.state_hash = bool(state_hash)

    def astuple(self):
        return tuple(getattr(self, k) for k in self.FIELDS)

    def __eq__(self, other):
        return type(other) is type(self) and self.astuple() == other.astuple() and self.state_hash == other.state_hash

    def __repr__(self):
        return "FileHeader(" + ", ".join(f"{k}={getattr(self, k)}" for k in self.FIELDS) + (", state_hash=True" if self.state_hash else "") + ")"

    def pack(self):
        self.check()
        return _HEADER.pack(self.MAGIC, VERSION | (STATE_HASH_BIT if self.state_hash else 0), *self.astuple())

    @classmethod
    def unpack(cls, data):
        if len(data) < HEADER_BYTES:
            raise ValueError(f"truncated file: the header is {HEADER_BYTES} bytes, got {len(data)}")
        magic, version, *rest = _HEADER.unpack(data[:HEADER_BYTES])
        if magic in cls.FOREIGN:
            raise ValueError(cls.FOREIGN[magic])
        if magic != cls.MAGIC:
            raise ValueError(f"not a {cls.NOUN}: magic {magic!r}, expected {cls.MAGIC!r}")
        if version & ~STATE_HASH_BIT != VERSION:
            raise ValueError(f"{cls.NOUN} version {version & ~STATE_HASH_BIT}, this module reads version {VERSION}")
        hdr = cls(state_hash=bool(version & STATE_HASH_BIT), **dict(zip(cls.FIELDS, rest)))
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
        self.check_models()

    def check_models(self):
        """ValueError unless the eight model fields name kinds this format knows, and a P-frame model when the file has P frames"""
        raise NotImplementedError

    def types(self):
        return frame_types(self.frames, self.gop, bool(self.all_intra))


def _check_sides(h, w):
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f"4:2:0 frames have even sides >= 2, got {w} x {h}")


# ---- frames, GOPs and records --------------------------------------------------------------------------------------------------
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


def gop_starts(types):
    """per frame, the index of its GOP's I frame"""
    out, last = [], 0
    for i, t in enumerate(types):
        last = i if t == "I" else last
        out.append(last)
    return out


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


# ---- the state-hash trailer ----------------------------------------------------------------------------------------------------
class StateMismatch(ValueError):
    """a decoded frame's conditioning state is not the one the encoder hashed: .frame, .gop_start (the index of its GOP's I frame),
    .want (the file's hash) and .got (the decoder's), both ints in [0, 2^64)"""

    def __init__(self, frame, gop_start, want, got):
        super().__init__(f"state mismatch at frame {frame} (its GOP starts at frame {gop_start}): the file says {want:016x}, this decoder "
                         f"computed {got:016x}; nothing decoded from this state on can be trusted")
        self.frame, self.gop_start, self.want, self.got = int(frame), int(gop_start), int(want), int(got)


def trailer_bytes(hashes):
    """the trailer of a hashed file: one big-endian u64 per frame in display order"""
    return struct.pack(f">{len(hashes)}Q", *hashes)


def split_trailer(data, hdr, header_bytes=HEADER_BYTES):
    """(header + records, state hashes) of the whole file `data`: the trailer is the last 8 * frames bytes of a hashed file (hdr.state_hash)
    -> (data, None) for an un-hashed one.  ValueError when a hashed file has no room for its trailer; a trailer of another length shows
    as records that end early or late (`hashed_record_ranges`)."""
    if not hdr.state_hash:
        return data, None
    n = 8 * hdr.frames
    if len(data) < header_bytes + n:
        raise ValueError(f"truncated file: a state-hash trailer of {n} bytes ({hdr.frames} frames) does not fit {len(data) - header_bytes} bytes "
                         "behind the header")
    return data[:len(data) - n], list(struct.unpack_from(f">{hdr.frames}Q", data, len(data) - n))


def hashed_record_ranges(data, hdr, header_bytes=HEADER_BYTES):
    """record_ranges over the file without its trailer -> (ranges, state hashes or None).  ValueError when the records do not end
    exactly where the trailer (or, in an un-hashed file, the file's end) begins."""
    body, hashes = split_trailer(data, hdr, header_bytes)
    try:
        return record_ranges(body, hdr.frames, header_bytes), hashes
    except ValueError as e:
        if hashes is None:
            raise
        raise ValueError(f"the state-hash trailer is not the {8 * hdr.frames} bytes behind the last record: {e}") from None


def read_state_hashes(data, header_cls):
    """the state hashes of a sequence file (its bytes) of the format `header_cls`: a list of `frames` ints in display order, or None for
    an un-hashed file; ValueError for a file whose trailer does not sit right behind its last record"""
    data = bytes(data)
    return hashed_record_ranges(data, header_cls.unpack(data))[1]


class VerifyReport:
    """what verify_sequence returns, kept while it walks: every GOP is an independent chain, so a GOP is abandoned at its first
    mismatch (what follows would be decoded under a wrong condition) and the others go on"""

    def __init__(self, hdr, starts, want):
        self.frames, self.starts, self.want = hdr.frames, starts, want
        self.checked, self.mismatches, self.dead = 0, [], {}                         # dead: a given-up GOP's I frame -> its bad frame

    def abandoned(self, index):
        return self.starts[index] in self.dead

    def check(self, index, got):
        """note frame `index` as checked; a hash that is not the file's is recorded and gives the frame's GOP up"""
        self.checked += 1
        if got != self.want[index]:
            self.mismatches.append({"frame": index, "gop_start": self.starts[index], "want": self.want[index], "got": got})
            self.dead[self.starts[index]] = index

    def result(self):
        """-> {"frames": n, "checked": frames hashed, "mismatches": [{"frame", "gop_start", "want", "got"}], "unchecked": [frames skipped
        behind a mismatch]}, indices ascending"""
        unchecked = [i for i in range(self.frames) if self.abandoned(i) and i > self.dead[self.starts[i]]]
        return {"frames": self.frames, "checked": self.checked, "mismatches": sorted(self.mismatches, key=lambda m: m["frame"]),
                "unchecked": unchecked}


def print_report(report):
    """verify_sequence's report as one JSON line on stdout, hashes in hex -> the exit status: 0 when clean, 3 on any mismatch"""
    import json
    out = dict(report, mismatches=[dict(m, want=f"{m['want']:016x}", got=f"{m['got']:016x}") for m in report["mismatches"]])
    print(json.dumps(out))
    return 3 if report["mismatches"] else 0


# ---- the models against the header ---------------------------------------------------------------------------------------------
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


def check_side(role, model, coded, given, subject, widths="widths"):
    """One model against its side of the header: ValueError unless kind, widths and fingerprint agree.  role: "I-frame" | "STEM" |
    "P-frame"; coded = (kind, its name, (a, b), fingerprint) from the file, given = (kind, its name, (a, b)) of `model`; subject and
    `widths` word the widths' refusal ("the file's <subject> has <widths> (a, b)")."""
    (kind, name, ab, crc), (kind_in, name_in, ab_in) = coded, given
    if kind_in != kind:
        raise ValueError(f"the file was coded with {name}, the {role} model passed in is {name_in}")
    if tuple(ab_in) != tuple(ab):
        raise ValueError(f"the file's {subject} has {widths} ({ab[0]}, {ab[1]}), the model passed in ({ab_in[0]}, {ab_in[1]})")
    got = fingerprint(model)
    if got != crc:
        raise ValueError(f"the {role} model's weights or tables are not the ones the file was coded with (fingerprint {got:08x}, file {crc:08x})")


def open_for_decoding(src, header_cls, check_header, need_hashes=False):
    """Everything decode_sequence and verify_sequence know before the first record is decoded, in the one order of the module
    docstring: the file (header, records, trailer), then check_header(hdr) -- the models --, then, with need_hashes, the refusal of an
    un-hashed file.  -> (header, the file's bytes, record ranges, the trailer's hashes or None, frame types, gop_starts)"""
    data = _read_all(src)
    hdr = header_cls.unpack(data)
    ranges, hashes = hashed_record_ranges(data, hdr)
    check_header(hdr)
    if need_hashes and hashes is None:
        raise ValueError("the file carries no state hashes (it was written without state_hash=True): nothing to verify it against")
    types = hdr.types()
    return hdr, data, ranges, hashes, types, gop_starts(types)


# ---- sources and sinks ---------------------------------------------------------------------------------------------------------
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


def _read_all(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    fd, close = _open(src, "rb")
    try:
        return fd.read()
    finally:
        if close:
            fd.close()


def _planes_bytes(planes):
    from . import data
    buf = io.BytesIO()
    data._write_planes(buf, planes, append=True)
    return buf.getvalue()


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------
def _state_dict(path):
    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd and not any(torch.is_tensor(v) for v in sd.values()):
        sd = sd["state_dict"]
    if not isinstance(sd, dict) or not sd or not all(torch.is_tensor(v) for v in sd.values()):
        raise ValueError(f"{path} holds no state_dict")
    return sd


def load_sized(cls_name, path, device, n_key, m_key):
    """the class `cls_name` of models/ built as cls(N, M) and loaded from the checkpoint at `path` (a state_dict, tables included):
    N is the first extent of the tensor at `n_key`, M half that of the one at `m_key`"""
    from . import models
    sd = _state_dict(path)
    try:
        net = getattr(models, cls_name)(sd[n_key].size(0), sd[m_key].size(0) // 2)
        net.load_state_dict(sd)
    except (KeyError, RuntimeError) as e:
        raise ValueError(f"{path} is no checkpoint of {cls_name}: {e}") from e
    return net.to(device).eval()


# ---- the command line ----------------------------------------------------------------------------------------------------------
def add_common_options(sub, i_option, i_help, p_option, p_help):
    """the sub-commands encode, decode and verify under `sub`, with the options all three share; the two models are named by
    --<i_option> / --<p_option>, each with its -checkpoint -> the three parsers by name"""
    for name in ("encode", "decode", "verify"):
        s = sub.add_parser(name)
        s.add_argument(f"--{i_option}", required=True, help=i_help)
        s.add_argument(f"--{i_option}-checkpoint", required=True)
        s.add_argument(f"--{p_option}", default=None, help=p_help)
        s.add_argument(f"--{p_option}-checkpoint", default=None)
        s.add_argument("--input", required=True)
        if name != "verify":
            s.add_argument("--output", required=True)
        s.add_argument("--device", default="cuda:0")
    return sub.choices


def add_coding_options(encode, decode):
    """the options of `encode` and of `decode` that both codecs have"""
    encode.add_argument("--width", type=int, required=True)
    encode.add_argument("--height", type=int, required=True)
    encode.add_argument("--bit-depth", type=int, default=8)
    encode.add_argument("--frames", type=int, default=None, help="code the first so many frames")
    encode.add_argument("--gop", type=int, default=12)
    encode.add_argument("--all-intra", action="store_true")
    encode.add_argument("--quality", type=int, default=4)
    encode.add_argument("--state-hash", action="store_true", help="write a hashed file: every frame's conditioning state, checked while decoding")
    decode.add_argument("--frames", default=None, help="START:STOP, decode only these frames")
    decode.add_argument("--no-verify", action="store_true", help="do not check a hashed file's state hashes")


def parse_frame_range(text):
    """--frames START:STOP -> (start, stop); None -> None"""
    if text is None:
        return None
    try:
        start, stop = (int(v) for v in text.split(":"))
    except ValueError:
        raise ValueError(f"--frames is START:STOP, got {text!r}") from None
    return start, stop


def run_command(args, encode, decode, verify):
    """The sub-command of `args` around a codec's three entry points: encode(the input as a data.YUVSequence) -> encode_sequence's
    result, decode((start, stop) or None), verify() -> verify_sequence's report.  Prints the result line -> the exit status."""
    if args.command == "encode":
        from . import data
        res = encode(data.YUVSequence(args.input, args.width, args.height, args.bit_depth, frames=args.frames, device=args.device))
        print(f"{len(res['frames'])} frames, {res['bytes']} bytes, {res['bpp_ave']:.6f} bpp")
    elif args.command == "verify":
        return print_report(verify())
    else:
        decode(parse_frame_range(args.frames))
        print(f"decoded {args.input} into {args.output}")
    return 0


def exit_status(run, args):
    """run(args) -> its exit status; 2 after a refusal (ValueError), whose message goes to stderr; 3 when a state hash did not match"""
    try:
        return run(args)
    except StateMismatch as e:
        print(f"mismatch: {e}", file=sys.stderr)
        return 3
    except ValueError as e:
        print(f"refused: {e}", file=sys.stderr)
        return 2
