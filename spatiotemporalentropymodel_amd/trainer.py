"""The P-frame optimisation step of stem/trainSTEM.py:203-218 as ONE explicit launch schedule (no torch autograd, no
torch elementwise kernels):

    zero main gradients -> STEM forward with the fused glue (engine.forward(rate_coef=...): EMLoss value and
    d loss / d likelihood come out of the forward) -> engine.backward -> [data-parallel exchange] -> global norm ->
    clip + Adam -> auxiliary loss + quantile gradient -> aux Adam

~65 launches instead of ~160 through nn.Module / autograd / torch.optim (selfcheck.p_frame_step, the generic route every
parity test against the reference's goldens goes through; tests/test_hip_trainer.py ties this route to it: same Philox
noise -> same likelihoods, gradients and updated parameters).  The arithmetic is the same kernels; what disappears is
the per-dispatch latency of ~50 few-microsecond glue kernels per step and most of the host time.

Only `EMLoss` (rate-only, the trainSTEM criterion) has this closed form; other criteria use the generic route.

`image_step` is the image-side counterpart: one batch of compressai_examples/train.py's loop for an I-frame model of the zoo, on the
layer-wise autograd Functions (every launch a HIP kernel; no schedule of its own).

What steers those loops is here too: `validate` (the validation pass of stem/trainSTEM.py:265-295, on engine.eval_rate's fused eval
glue or module by module), `fit` (the epoch loop of :172-262 around a SeptupletTrainer: validation every N P-frame steps from its
`on_step` hook, scheduler step, best-loss and periodic checkpoints, `resume_state`), `validate_pixel` (stem_roi/train_stem_roi.py
:348-391 and :658-716) and `validate_image` (compressai_examples/train.py:179-207).
"""
from __future__ import annotations

import contextlib
import math
import os

import torch

from . import config as _config
from . import functional as F
from .layers import join_wgrad_stream


#: the stream set-up bench.py measures; the environment variables of the same names override them ("" disables).
#: Round 5: 160 of the 256 CUs for the latent prefetch (192 until round 4): the P-frame step got shorter and its three streams now
#: keep the chip busier, 11.75 against 11.99 ms per bench step (128: 12.15, 144: 12.07, 176: 11.83, 224: 12.10, no mask: 12.08;
#: profiles/r05_ab_cumask*.log)
SCHEDULE_DEFAULTS = {"STEM_STREAM_PRIO": "latents=0,side=-1,compute=-1", "STEM_STREAM_CUMASK": "latents=block:160"}


def tuned_schedule(device):
    """-> a context manager that makes a high-priority compute stream current.  Call it BEFORE anything creates a stream (the
    first FusedPFrameStep / LatentPrefetcher / engine call), enter it around the training loop:

        sched = tuned_schedule(dev)
        fused, pf = FusedPFrameStep(stem, opt, aux_opt), LatentPrefetcher(imodel)
        with sched:
            for frames in loader: ...

    Installs the stream priorities and the CU mask of SCHEDULE_DEFAULTS unless the environment already sets them: the P-frame
    step's own streams at HIP's high priority, the latent-prefetch stream at normal priority and confined to 192 of the 256 CUs,
    so that the step's short kernels never queue behind running workgroups of the long analysis-transform kernels.  Scheduling
    only: no result depends on it."""
    for k, v in SCHEDULE_DEFAULTS.items():
        os.environ.setdefault(k, v)                    # config.runtime() parses them (fields stream_prio / stream_cumask)
    F.make_stream(device, "side")                      # parses STEM_STREAM_PRIO once
    if "compute" in (F._STREAM_PRIO or {}):
        return torch.cuda.stream(F.make_stream(device, "compute"))
    return contextlib.nullcontext()


class LatentPrefetcher:
    """Latents of the frozen I-frame model (getY, compressai priors.py:686-694; frozen in stem/trainSTEM.py:128) computed on their
    own stream, ahead of the P-frame steps that consume them.  The reference calls getY(frame t) inside the loop over the
    frames (stem/trainSTEM.py:171-179); the transform does not depend on the STEM weights, so frame t + `ahead`'s latents can be
    in flight while P-step t runs: their long matrix kernels fill the stretches where a P-frame step cannot use the chip (norm
    reduction -> clip -> Adam -> weight packing, and the small 4x4 / 8x8 layers).

        pf = LatentPrefetcher(imodel)
        pf.start(frames)                      # enqueues frames 0 .. ahead
        for t in range(1, len(frames)):
            y_cur, _ = pf.get(t)              # compute stream waits for frame t's event; frame t + ahead is enqueued
            ...

    Across sequences (a training loop whose loader holds the next batch): `pf.start(frames, next_frames=following)` also computes
    the following sequence's first two latents during this sequence's last two P-frame steps; `pf.start(following, ...)` adopts them.
    """

    def __init__(self, imodel, ahead=1):
        self.imodel, self.ahead = imodel, int(ahead)
        self._stream = None
        self._frames = self._ys = self._events = None
        self._next = 0
        self._nxt = None            # {"frames", "ys", "events", "n"}: the FOLLOWING sequence, whose first latents are computed early

    def _enqueue_into(self, frames, ys, events, t):
        dev = frames[t].device
        if self._stream is None or self._stream.device != dev:
            self._stream = F.make_stream(dev, "latents")
        with F.on_stream(self._stream), torch.no_grad():
            ys[t] = self.imodel.getY(frames[t])
            events[t] = torch.cuda.Event()
            events[t].record(self._stream)

    def _enqueue(self, t):
        self._enqueue_into(self._frames, self._ys, self._events, t)

    def start(self, frames, frames_ready=False, next_frames=None):
        """frames_ready=True: the frame tensors are not being written by work queued on the compute stream (a data loader's
        finished batch), so the first transforms need not wait for what that stream still has queued -- they then overlap the
        tail of the previous optimisation step.

        next_frames: the sequence that will be started NEXT (the loader's following batch, already resident).  A sequence cannot
        begin its first P-frame step before the latents of its frames 0 and 1 exist -- two analysis transforms (~1.5 ms at the
        bench size) during which the step's own streams idle.  With next_frames those two are computed during the LAST two
        P-frame steps of this sequence, like every other frame's, and start(next_frames) then finds them in flight.  The transform
        is frozen (stem/trainSTEM.py:128) and the calls keep their order (this sequence's frames, then the next one's), so every
        result -- noise draws included -- is what the unpipelined loop computes."""
        frames = list(frames) if not isinstance(frames, list) else frames
        n = len(frames)
        adopted = 0
        if self._nxt is not None and (self._nxt["frames"] is frames or
                                      (len(self._nxt["frames"]) == n and all(a is b for a, b in zip(self._nxt["frames"], frames)))):
            self._ys, self._events, adopted = self._nxt["ys"], self._nxt["events"], self._nxt["n"]
        else:
            self._ys, self._events = [None] * n, [None] * n
        self._frames = frames
        self._nxt = None
        if next_frames is not None:
            nf = list(next_frames) if not isinstance(next_frames, list) else next_frames
            self._nxt = {"frames": nf, "ys": [None] * len(nf), "events": [None] * len(nf), "n": 0}
        dev = self._frames[0].device
        if self._stream is None or self._stream.device != dev:
            self._stream = F.make_stream(dev, "latents")
        if not frames_ready:
            F.stream_wait(self._stream, F.cur_stream(dev))      # the frames were produced on the compute stream
        self._next = adopted
        while self._next < n and self._next <= self.ahead:
            self._enqueue(self._next)
            self._next += 1
        return self

    def get(self, t):
        """(y, y + noise) of frame t, ordered before whatever the current stream does next"""
        n = len(self._frames)
        while self._next < n and self._next <= t + self.ahead:
            self._enqueue(self._next)
            self._next += 1
        if self._nxt is not None and self._next >= n:
            # positions beyond this sequence: the next one's opening frames, one more than `ahead` (a sequence opens with TWO latents)
            want = min(t + self.ahead + 2 - n, self.ahead + 1, len(self._nxt["frames"]))
            while self._nxt["n"] < want:
                self._enqueue_into(self._nxt["frames"], self._nxt["ys"], self._nxt["events"], self._nxt["n"])
                self._nxt["n"] += 1
        cur = F.cur_stream(self._frames[t].device)
        cur.wait_event(self._events[t])
        y, yq = self._ys[t]
        y.record_stream(cur)
        yq.record_stream(cur)
        return y, yq


class LazyScalar:
    """A scalar that the step left in device memory on the auxiliary stream: a private copy (later steps do not overwrite it)
    plus the event after which it is valid.  float() / tensor() wait for that event -- no host synchronisation unless
    somebody looks at the value."""

    def __init__(self, value, event, scale=1.0, sqrt=False):
        self._v, self._e, self._scale, self._sqrt = value, event, scale, sqrt

    def tensor(self):
        cur = F.cur_stream(self._v.device)
        cur.wait_event(self._e)
        self._v.record_stream(cur)          # allocated on the auxiliary stream, read here: the allocator must not recycle it under this reader
        v = self._v.reshape(())
        return (v.sqrt() if self._sqrt else v) * self._scale if (self._sqrt or self._scale != 1.0) else v

    def __float__(self):
        return float(self.tensor())


class FusedPFrameStep:
    def __init__(self, stem, optimizer, aux_optimizer):
        self.stem, self.opt, self.aux_opt = stem, optimizer, aux_optimizer
        self.eng = stem.engine()
        eb = stem.entropy_bottleneck
        if eb.quantiles.grad is None or getattr(eb.quantiles, "_flat_grad_view", None) is None:
            raise ValueError("FusedPFrameStep needs the flat-buffer optimisers of optim.configure_optimizers(fused=True)")
        self._aux_loss = torch.zeros(1, dtype=torch.float32, device=eb.quantiles.device)
        self._grad_clean = False          # True once our own Adam pass has cleared the flat gradient buffer
        #: clear the gradient buffer inside the Adam pass (saves the 72 MB memset of the next step); set False to leave the
        #: gradients in place after step() for inspection -- they are then zeroed at the start of the next step instead
        self.clear_grad_in_adam = True
        #: this schedule produces every gradient exactly once per step, so its backward OVERWRITES the flat gradient buffer instead
        #: of adding into a cleared one (engine.accumulate_grads = False for the backward): no clearing inside the Adam pass (72 MB
        #: written) and no read of the old values by the slab sums (72 MB read) -- and the gradients stay in place after step() for
        #: inspection.  False restores the clear-then-accumulate form (`clear_grad_in_adam` then decides where the clearing happens)
        self.overwrite_grads = _config.runtime().trainer_overwrite_grads
        #: the optimiser pass leaves per-chunk maxima of the updated parameters for the fp16 weight packing (no maximum launches)
        self.adam_block_max = _config.runtime().adam_block_max
        # the auxiliary work (one workgroup of latency-bound launches after the optimiser pass) shares the weight-gradient stream, which
        # is idle then: one high-priority stream less (compute, hyper branch, weight gradients + this, and the process group's own
        # = the four hardware queues of that priority; with a fifth the one-rank RCCL run took 14.86 instead of 14.69 ms per step)
        self._aux_stream = self.eng.side_stream(eb.quantiles.device) or F.make_stream(eb.quantiles.device, "side")
        self._aux_pending = False
        self._tail_plan = None            # the ordered optimiser tail of the latest ordinary step (engine.StemEngine.tail_plan), or None
        self._done_event = torch.cuda.Event()           # re-recorded every step: the LazyScalars of the LATEST step wait on it

    def step(self, y_cur, y_cond, num_pixels, grad_scale=1.0, reducer=None):
        """y_cur / y_cond: the frame's and the conditioning latents [B,C,h,w]; num_pixels = N*H*W of the FRAMES (EMLoss
        normalisation).  Returns (out, criterion_out, aux_loss, grad_norm) like selfcheck.p_frame_step; the loss entries
        are 0-dim fp64 device tensors; aux_loss and grad_norm are LazyScalars (private copies, valid whenever they are read).
        Call finish() before reading `entropy_bottleneck.quantiles` / the aux optimiser outside of step()."""
        stem, opt, aux_opt, eng = self.stem, self.opt, self.aux_opt, self.eng
        eb = stem.entropy_bottleneck
        overwrite = bool(self.overwrite_grads)                      # (the data-parallel reducers sum in place: unaffected)
        if overwrite or (self._grad_clean and opt._dev is None):    # nothing to clear / cleared by the previous step's Adam pass
            for p in opt.flat.params:
                p.grad = p._flat_grad_view
        else:
            opt.flat.zero_grad()                                    # one memset; the aux gradient is overwritten below
        coef = -1.0 / (math.log(2.0) * num_pixels)
        y_hat, lik_y, lik_z, k = eng.forward(y_cur, y_cond, True, rate_coef=(coef, -1.0 / num_pixels))
        eng.accumulate_grads = not overwrite
        try:
            eng.backward(k, k["dlik_y"], k["dlik_z"])               # an attached OverlappedGradReducer exchanges slices in here
        finally:
            eng.accumulate_grads = True
        if reducer is not None:
            F.tape_py(reducer.finish if hasattr(reducer, "finish") else reducer.all_reduce)
        join_wgrad_stream()
        main = F.cur_stream(y_hat.device)
        if self._aux_pending:                    # the previous step's auxiliary work reads the parameters Adam is about to change
            F.stream_wait(main, self._aux_stream)
            self._aux_pending = False
        F.sumsq(opt.flat.grad, opt._sumsq, overwrite=True)
        clean = opt._dev is None and self.clear_grad_in_adam and not overwrite
        use_bmax = opt._dev is None and eng.use_fx3 and self.adam_block_max
        # the tail in first-use order: the next forward's first kernels need TPM.0 / HE.0 (and the small tensors kernels read in
        # place) only -- that group runs here, the others on the auxiliary stream under the forward (engine.StemEngine.run_tail)
        plan = None
        if (use_bmax and eng.tail_ordered and eng.pack_pair and eng.side_stream(main.device) is self._aux_stream
                and not torch.cuda.is_current_stream_capturing()):
            opt.ensure_block_maxima()
            plan = eng.tail_plan(opt)
        self._tail_plan = plan
        if plan is not None:
            opt.begin_ranges(grad_scale)
            eng.run_tail(plan, lambda table: opt.step_ranges(table, zero_grad=clean))
        else:
            opt.step(grad_scale=grad_scale, norm_is_current=True, zero_grad=clean, block_max=use_bmax)
        self._grad_clean = clean
        # auxiliary loss on the UPDATED parameters (stem/trainSTEM.py:216-218); its gradient goes straight into the aux
        # optimiser's flat buffer (the only aux parameter is `entropy_bottleneck.quantiles`).  One workgroup of latency-bound
        # work on its own stream; the training forward does not read the quantiles, so nothing waits for it until the NEXT
        # optimiser step (above) or until the caller looks at the returned values (LazyScalar).
        F.stream_wait(self._aux_stream, main)
        with F.on_stream(self._aux_stream):
            # private copies (the persistent buffers are overwritten by the next step), made by a library call: recordable
            gn_copy = F.copy_d2d(torch.empty_like(opt._sumsq[:1]), opt._sumsq[:1])
            pack = F.eb_pack(eb._tensors14())
            F.eb_aux_loss_grad(eb.quantiles.detach(), pack, eb.target, eb.quantiles._flat_grad_view, loss_out=self._aux_loss)
            eb.quantiles.grad = eb.quantiles._flat_grad_view
            aux_opt.step()
            aux_copy = F.copy_d2d(torch.empty_like(self._aux_loss), self._aux_loss)
            done = self._done_event
            F.event_record(done, self._aux_stream)
        self._aux_pending = True
        # the next forward's weight packing, issued now; the fp16 images take their scales from the maxima the optimiser pass left
        eng.ensure_packed(block_max=(opt.block_maxima, opt.flat.data) if use_bmax else None)
        loss3 = k["loss3"]
        out = {"y_hat": y_hat, "likelihoods": {"y": lik_y, "z": lik_z}}
        oc = {"y_bpp_loss": loss3[0], "z_bpp_loss": loss3[1], "loss": loss3[2]}
        return out, oc, LazyScalar(aux_copy, done), LazyScalar(gn_copy, done, scale=grad_scale, sqrt=True)

    def after_replay(self):
        """host-side state a replayed step (tape.TapedPFrameStep) leaves as the ordinary one does: the weights changed (the packed
        copies' keys), the auxiliary stream holds work, the gradient buffer was cleared by the optimiser pass"""
        from .layers import bump_weight_epoch
        bump_weight_epoch(self.opt.flat.params)
        self._aux_pending = True
        if self._tail_plan is not None:          # the replay recorded the events of its ordered tail again: nobody has waited for these
            self.eng.mark_tail(self._tail_plan)

    def finish(self):
        """order everything the step left on its auxiliary stream before the current stream (end of training, checkpointing,
        evaluation: anything that reads `entropy_bottleneck.quantiles` or the aux optimiser's state -- or the parameters themselves:
        the later groups of an ordered optimiser tail run on that stream)"""
        if self._aux_pending:
            F.stream_wait(F.cur_stream(self._aux_loss.device), self._aux_stream)
            self._aux_pending = False


def subsample_septuplet(images, rand):
    """The temporal subsampling of stem/trainSTEM.py:175-182: with probability 1/4 each, frames 1,3,5,7 / 1,4,7 / 1,7 / all seven
    of the septuplet (`rand` = the loop's random.random() draw)."""
    if rand <= 0.25:
        return images[0:7:2]
    if rand <= 0.50:
        return images[0:7:3]
    if rand <= 0.75:
        return images[0:7:6]
    return images


class SeptupletTrainer:
    """The loop body of stem/trainSTEM.py:174-226 for ONE loader item (a septuplet: list of 7 frame batches [B,3,H,W]) -- the unit
    BASELINE.json's metric counts and `bench.py` times:

        frames = subsample_septuplet(images, random.random())          # :175-182
        _, y_condition = IFrameCompressor.getY(frames[0])              # :199 (frozen I-frame model, :128)
        for every later frame:  y_cur = getY(frame) -> stem(y_cur, y_condition.detach()) -> y_condition = y_hat ->
                                criterion -> backward -> clip -> optimizer.step -> aux_loss.backward -> aux_optimizer.step   (:203-218)

    route "taped" (default): the explicit schedule FusedPFrameStep replayed from its launch tape; "fused": the explicit schedule
    issued launch by launch; "generic": nn.Module / autograd / optimiser calls (selfcheck.p_frame_step), which needs `criterion`.
    prefetch: getY of frame t + `ahead` on its own stream while step t runs (LatentPrefetcher); otherwise all latents first.
    reducer / grad_scale: data parallel (distributed.OverlappedGradReducer attached to stem.engine(), 1 / world).
    `rng`: a random.Random for the subsampling draw (seed it per rank and per epoch as the training script seeds `random`)."""

    def __init__(self, imodel, stem, optimizer, aux_optimizer, *, route="taped", prefetch=True, ahead=1, reducer=None, grad_scale=1.0,
                 criterion=None, rng=None):
        import random
        self.imodel, self.stem, self.opt, self.aux_opt = imodel, stem, optimizer, aux_optimizer
        self.route, self.reducer, self.grad_scale, self.criterion = route, reducer, float(grad_scale), criterion
        self.rng = rng or random.Random(0)
        self.step_fn = None
        if route in ("taped", "fused"):
            self.step_fn = FusedPFrameStep(stem, optimizer, aux_optimizer)
            if route == "taped":
                from .tape import TapedPFrameStep
                self.step_fn = TapedPFrameStep(self.step_fn)
        elif route != "generic":
            raise ValueError(f"SeptupletTrainer: unknown route {route!r}")
        elif criterion is None:
            raise ValueError("SeptupletTrainer: the generic route needs the criterion module")
        self.prefetch = LatentPrefetcher(imodel, ahead=ahead) if prefetch else None
        self.on_step = None             # called after every P-frame step with (t, out, criterion_out, aux, grad_norm)

    def train_septuplet(self, images, rand=None, next_images=None, frames_ready=True):
        """One loader item.  rand: the subsampling draw (None: self.rng.random(); 1.0 keeps all seven frames).  next_images: the
        FOLLOWING item's (already subsampled) frames, whose first two latents are then computed during this item's last steps.
        Returns [(criterion_out, aux, grad_norm)] of the P-frame steps (device-resident values; no host synchronisation)."""
        frames = list(subsample_septuplet(list(images), self.rng.random() if rand is None else rand))
        num_pixels = frames[0].shape[0] * frames[0].shape[-2] * frames[0].shape[-1]
        if self.prefetch is not None:
            self.prefetch.start(frames, frames_ready=frames_ready, next_frames=next_images)
            ys = None
            y_cond = self.prefetch.get(0)[1]
        else:
            with torch.no_grad():
                ys = [self.imodel.getY(f) for f in frames]
            y_cond = ys[0][1]
        log = []
        for t in range(1, len(frames)):
            y_cur = self.prefetch.get(t)[0] if self.prefetch is not None else ys[t][0]
            if self.step_fn is not None:
                out, oc, aux, gn = self.step_fn.step(y_cur, y_cond, num_pixels, grad_scale=self.grad_scale, reducer=self.reducer)
            else:
                from .selfcheck import p_frame_step
                out, oc, aux, gn = p_frame_step(self.imodel, self.stem, self.criterion, self.opt, self.aux_opt, frames[t], y_cond,
                                                grad_scale=self.grad_scale, reducer=self.reducer, y_cur=y_cur)
            y_cond = out["y_hat"]
            log.append((oc, aux, gn))
            if self.on_step is not None:
                self.on_step(t, out, oc, aux, gn)
        return log

    def finish(self):
        if self.step_fn is not None:
            self.step_fn.finish()

    def validate(self, loader, **kw):
        """`validate` (below; stem/trainSTEM.py:265-295) on this trainer's models, between two P-frame steps -- also in the middle of a
        septuplet, from `on_step`, where the reference calls it (:228-231).  The step's auxiliary stream is joined first (the eval
        forward reads the quantiles the auxiliary optimiser writes); the pass has a prefetcher of its own, kept for the next pass;
        nothing the next step reads -- parameters, optimiser states, noise offsets, the training prefetcher's latents, a recorded
        tape's buffers -- is written.  A `criterion` given to the trainer serves the generic route."""
        self.finish()
        if hasattr(self.step_fn, "packs_are_current"):
            self.step_fn.packs_are_current()
        if kw.get("prefetch", True) is True and self.prefetch is not None:
            if getattr(self, "_val_prefetch", None) is None:
                self._val_prefetch = LatentPrefetcher(self.imodel, ahead=self.prefetch.ahead)
            kw["prefetch"] = self._val_prefetch
        elif kw.get("prefetch", True) is True:
            kw["prefetch"] = False
        if self.criterion is not None:
            kw.setdefault("criterion", self.criterion)
        return validate(self.imodel, self.stem, loader, **kw)


def image_step(model, criterion, optimizer, aux_optimizer, x, clip_max_norm=1.0):
    """One batch of compressai_examples/train.py:127-143 for an I-frame model of the zoo:

        zero both gradients -> model(x) -> criterion -> loss.backward() -> clip_grad_norm_(all parameters, clip_max_norm) ->
        optimizer.step() -> model.aux_loss().backward() -> aux_optimizer.step()

    criterion: losses.RateDistortionLoss; (optimizer, aux_optimizer): optim.configure_optimizers(model, args, max_norm=None) -- the
    clipping is optim.clip_grad_norm_ over both flat gradient buffers, as the script clips model.parameters() (the quantiles get no
    gradient from the main loss; their zeros join the norm).  The reference's torch.optim.Adam pair (fused=False) works too.
    -> (out_criterion, aux_loss, grad_norm): device-resident values, no host synchronisation; grad_norm is the norm before
    clipping, None with clip_max_norm <= 0."""
    from .layers import to_nchw
    from .optim import clip_grad_norm_
    optimizer.zero_grad()
    aux_optimizer.zero_grad()
    out_net = model(x)
    if F.nhwc_ld(out_net["x_hat"]) is not None and not out_net["x_hat"].is_contiguous():
        out_net = dict(out_net, x_hat=to_nchw(out_net["x_hat"]))          # the criterion reads NCHW: the layout kernel, both ways
    out_criterion = criterion(out_net, x)
    out_criterion["loss"].backward()
    grad_norm = None
    if clip_max_norm > 0:
        if hasattr(optimizer, "flat"):
            grad_norm = clip_grad_norm_((optimizer, aux_optimizer), clip_max_norm)
        else:
            join_wgrad_stream()
            grad_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), clip_max_norm)
    optimizer.step()
    aux_loss = model.aux_loss()
    aux_loss.backward()
    aux_optimizer.step()
    return out_criterion, aux_loss, grad_norm


# ----------------------------------------------------------------------------- validation passes
@contextlib.contextmanager
def _eval_modes(*models):
    """the models in eval() inside, the `training` flag of every module as found on entry afterwards (also when the body raises).
    The reference's validation functions end with .train() on both models whatever they were (stem/trainSTEM.py:292-293); a frozen
    I-frame model (:128) stays frozen here."""
    modes = [(mod, mod.training) for m in models for mod in m.modules()]
    try:
        for m in models:
            m.eval()
        yield
    finally:
        for mod, flag in modes:
            mod.training = flag


@contextlib.contextmanager
def _noise_offsets_kept(*models):
    """A validation pass leaves the counter-based noise streams where it found them: mbt2018's getY draws noise in eval mode too
    (priors.py:691), which would otherwise shift every later training draw by the size of the test set.  The pass's own draws are
    a function of the offsets at entry: deterministic, the same on every rank."""
    kept = [(mod, mod._noise_offset) for m in models for mod in m.modules() if hasattr(mod, "_noise_offset")]
    try:
        yield
    finally:
        for mod, off in kept:
            mod._noise_offset = off


def _stem_route(stem, route):
    if route not in (None, "fused", "generic"):
        raise ValueError(f"validate: unknown route {route!r}")
    if route == "generic":
        return None
    if route is None and DEFAULT_VALIDATION_ROUTE != "fused":
        return None
    if route is None and tuple(stem.entropy_bottleneck.filters) != (3, 3, 3, 3):
        return None                                  # no engine for this bottleneck: the module route
    return stem.engine()                             # route="fused" on such a model: the engine's ValueError


#: what validate(route=None) means for a model that has an engine: "fused" only while tools/validation_bench.py finds the fused pass
#: at batch 1 not slower than the generic one beyond the run-to-run band (profiles/validation.json; the table and the reading of it
#: are in DESIGN.md section 7), "generic" otherwise
DEFAULT_VALIDATION_ROUTE = "fused"


def validate(imodel, stem, loader, *, criterion=None, route=None, prefetch=True, lr_scheduler=None, max_items=None):
    """The validation pass of stem/trainSTEM.py:265-295: both models in eval mode, under no_grad, over every item of `loader` (a
    list of frame batches [B,3,H,W], any length >= 2):

        _, y_cond = getY(frame 0);   for every later frame:  y_cur, _ = getY(frame) -> P step -> y_cond = y_hat

    -> {"loss", "y_bpp_loss", "z_bpp_loss", "count"} (Python floats): the means of EMLoss over the P steps, each step weighted with
    its batch size B -- the per-sample mean, i.e. what the reference's batch-1 test loader (:148) computes, whatever the loader's
    batch size and however ragged its last batch; count = samples x P frames.

    route "fused": engine.eval_rate (the elementwise work of a step in 4 kernels, the sums in a device accumulator); "generic": the
    module call plus `criterion` (default losses.EMLoss()), the sums fp64 device tensors; None: DEFAULT_VALIDATION_ROUTE where the
    model has an engine, else generic.  Either way the host reads the device ONCE, at the end.
    prefetch: the latents through a LatentPrefetcher of this pass's own (a training loop's prefetcher keeps the next sequence's
    opening latents it has already computed); a LatentPrefetcher instance is used as it is (a caller that validates repeatedly).  max_items: stop after that many loader items.
    lr_scheduler: lr_scheduler.step(loss) at the end (:290).  Noise offsets and module modes are restored on exit.
    Data parallel: every rank validates the whole set; the pass is deterministic, so the ranks' schedulers agree."""
    eng = _stem_route(stem, route)
    if eng is None and criterion is None:
        from .losses import EMLoss
        criterion = EMLoss()
    pf = prefetch if isinstance(prefetch, LatentPrefetcher) else (LatentPrefetcher(imodel) if prefetch else None)
    acc = None
    with torch.no_grad(), _eval_modes(imodel, stem), _noise_offsets_kept(imodel, stem):
        for n, images in enumerate(loader):
            if max_items is not None and n >= max_items:
                break
            frames = list(images)
            if len(frames) < 2:
                raise ValueError(f"validate: loader item {n} has {len(frames)} frame(s); a P step needs two")
            B, _, H, W = frames[0].shape
            if acc is None:
                acc = torch.zeros(4, dtype=torch.float64, device=frames[0].device)
            if pf is not None:
                pf.start(frames, frames_ready=True)
                y_cond = pf.get(0)[1]
            else:
                y_cond = imodel.getY(frames[0])[1]
            for t in range(1, len(frames)):
                y_cur = pf.get(t)[0] if pf is not None else imodel.getY(frames[t])[0]
                if eng is not None:
                    y_cond = eng.eval_rate(y_cur, y_cond, B * H * W, acc=acc, weight=float(B))[0]
                else:
                    out = stem(y_cur, y_cond)
                    oc = criterion(out, frames[t])
                    y_cond = out["y_hat"]
                    acc += float(B) * torch.stack([oc["y_bpp_loss"].double().reshape(()), oc["z_bpp_loss"].double().reshape(()),
                                                   oc["loss"].double().reshape(()), torch.ones((), dtype=torch.float64, device=acc.device)])
    if acc is None:
        raise ValueError("validate: the loader is empty")
    a = acc.cpu().tolist()                               # the pass's one device-to-host copy
    res = {"y_bpp_loss": a[0] / a[3], "z_bpp_loss": a[1] / a[3], "loss": a[2] / a[3], "count": a[3]}
    if lr_scheduler is not None:
        lr_scheduler.step(res["loss"])
    return res


def _nchw_x_hat(out_net):
    """the model's output with x_hat as a plain NCHW batch (an image model of the zoo returns NHWC memory): the criterion and the next
    frame's analysis transform read NCHW -- the layout kernel, as in image_step"""
    from .layers import to_nchw
    if F.nhwc_ld(out_net["x_hat"]) is not None and not out_net["x_hat"].is_contiguous():
        return dict(out_net, x_hat=to_nchw(out_net["x_hat"]))
    return out_net


def _mean_dict(sums, cnt):
    vals = torch.stack([v.double().reshape(()) for v in sums.values()]).cpu().tolist()       # one copy per loader
    return {k: v / cnt for k, v in zip(sums, vals)}


def validate_pixel(model_i, model_p, loaders, criterion, *, criterion_rd=None):
    """The validation passes of the pixel-domain models (stem_roi/train_stem_roi.py):

    loaders = ONE loader of frame lists: _validation_stem_baseline (:348-391) -- frame 0 through model_i(x), later frames through
    model_p(x, x_conditioned), criterion(out, x) for both, x_conditioned = out["x_hat"]; -> {"loss", "mse_loss", "bpp_loss"}, the
    means over ALL frames (the I frame counts).
    loaders = a list / tuple of loaders of (frames, Qmap), one per quality level: _validation_stem_roi (:658-716) -- the quality map
    goes to both models, criterion(out, x, quality2lambda(Qmap)), and criterion_rd (default losses.RateDistortionLoss()) supplies
    the unweighted "mse"; -> one dictionary per loader, in order.

    Existing forwards and criteria only.  The sums stay device tensors until a loader is finished; modes are restored as in
    `validate`, and so are the noise offsets."""
    # a list of loaders, unless it is ONE loader given as a list of items (an item is a list of frame tensors)
    first = loaders[0] if isinstance(loaders, (list, tuple)) and len(loaders) else None
    roi = isinstance(loaders, (list, tuple)) and not (isinstance(first, (list, tuple)) and len(first) and torch.is_tensor(first[0]))
    if roi and criterion_rd is None:
        from .losses import RateDistortionLoss
        criterion_rd = RateDistortionLoss()
    from .losses import quality2lambda
    results = []
    with torch.no_grad(), _eval_modes(model_i, model_p), _noise_offsets_kept(model_i, model_p):
        for loader in (loaders if roi else [loaders]):
            sums, cnt = {}, 0
            for item in loader:
                images, qmap = item if roi else (item, None)
                lmbdamap = quality2lambda(qmap) if roi else None
                x_cond = None
                for idx, x in enumerate(images):
                    if roi:
                        out = _nchw_x_hat(model_i(x, qmap) if idx == 0 else model_p(x, x_cond, qmap))
                        oc = criterion(out, x, lmbdamap)
                        vals = {"loss": oc["loss"], "mse_loss": oc["mse_loss"], "bpp_loss": oc["bpp_loss"], "mse": criterion_rd(out, x)["mse_loss"]}
                    else:
                        out = _nchw_x_hat(model_i(x) if idx == 0 else model_p(x, x_cond))
                        oc = criterion(out, x)
                        vals = {"loss": oc["loss"], "mse_loss": oc["mse_loss"], "bpp_loss": oc["bpp_loss"]}
                    x_cond = out["x_hat"]
                    for k, v in vals.items():
                        sums[k] = v.detach().double() if k not in sums else sums[k] + v.detach().double()
                    cnt += 1
            if not cnt:
                raise ValueError("validate_pixel: an empty loader")
            results.append(_mean_dict(sums, cnt))
    return results if roi else results[0]


def validate_image(model, loader, criterion):
    """test_epoch of compressai_examples/train.py:179-207 for an I-frame model of the zoo: the means over the loader's batches of
    criterion(model(x), x)'s "loss", "bpp_loss", "mse_loss" and of model.aux_loss() ("aux_loss").  Sums on the device, one copy."""
    sums, cnt = {}, 0
    with torch.no_grad(), _eval_modes(model), _noise_offsets_kept(model):
        for x in loader:
            oc = criterion(_nchw_x_hat(model(x)), x)
            vals = {"loss": oc["loss"], "bpp_loss": oc["bpp_loss"], "mse_loss": oc["mse_loss"], "aux_loss": model.aux_loss()}
            for k, v in vals.items():
                sums[k] = v.detach().double() if k not in sums else sums[k] + v.detach().double()
            cnt += 1
    if not cnt:
        raise ValueError("validate_image: an empty loader")
    return _mean_dict(sums, cnt)


# ----------------------------------------------------------------------------- the epoch loop
def fit(trainer, train_loader, test_loader, lr_scheduler, epochs, *, start_epoch=0, start_iterations=0, validate_every=20000, save=None,
        save_every_epochs=2, on_validation=None):
    """The epoch loop of stem/trainSTEM.py:172-262 around a SeptupletTrainer (or anything with train_septuplet(images), validate(loader,
    lr_scheduler=), on_step and finish()):

        for epoch in start_epoch .. epochs - 1:
            for images in train_loader:  trainer.train_septuplet(images)
                after EVERY P-frame step: iterations += 1; if iterations % validate_every == 0 (:226-228): the validation pass over
                test_loader with lr_scheduler.step(loss) (:231, :290) -- inside the septuplet, so a lowered learning rate applies to
                the very next step -- and, when the loss is the best so far, the checkpoint `save + f"checkpoint_best_epoch{epoch}.pth.tar"`
            if epoch % save_every_epochs == 0:  the checkpoint `save + f"checkpoint_epoch{epoch}.pth.tar"` (:250-262)

    Checkpoints go through utils.save_checkpoint with the reference's keys {"epoch", "iterations", "state_dict", "optimizer",
    "aux_optimizer", "lr_scheduler"} (the trainer's .stem / .opt / .aux_opt); save=None writes none.  start_epoch / start_iterations:
    `resume_state` of a loaded checkpoint.  on_validation(epoch, iterations, result, is_best) is called after every pass.
    -> {"iterations", "best_loss", "validations": [(epoch, iterations, loss)]}."""
    from .utils import save_checkpoint
    state = {"iterations": int(start_iterations), "best": float("inf"), "epoch": int(start_epoch), "log": []}

    def checkpoint(name):
        if save is None:
            return
        trainer.finish()
        save_checkpoint({"epoch": state["epoch"], "iterations": state["iterations"], "state_dict": trainer.stem.state_dict(),
                         "optimizer": trainer.opt.state_dict(), "aux_optimizer": trainer.aux_opt.state_dict(),
                         "lr_scheduler": lr_scheduler.state_dict()}, filename=save + name)

    def after_step(*step):
        if user_hook is not None:
            user_hook(*step)
        state["iterations"] += 1
        if validate_every and state["iterations"] % validate_every == 0:
            res = trainer.validate(test_loader, lr_scheduler=lr_scheduler)
            best = res["loss"] < state["best"]
            state["log"].append((state["epoch"], state["iterations"], res["loss"]))
            if best:
                state["best"] = res["loss"]
                checkpoint(f"checkpoint_best_epoch{state['epoch']}.pth.tar")
            if on_validation is not None:
                on_validation(state["epoch"], state["iterations"], res, best)

    user_hook = trainer.on_step
    trainer.on_step = after_step
    try:
        for epoch in range(int(start_epoch), int(epochs)):
            state["epoch"] = epoch
            for images in train_loader:
                trainer.train_septuplet(images)
            if save_every_epochs and epoch % save_every_epochs == 0:
                checkpoint(f"checkpoint_epoch{epoch}.pth.tar")
    finally:
        trainer.on_step = user_hook
    trainer.finish()
    return {"iterations": state["iterations"], "best_loss": state["best"], "validations": state["log"]}


def resume_state(checkpoint, stem, optimizer, aux_optimizer, lr_scheduler):
    """stem/trainSTEM.py:138-143: the three load_state_dict calls (plus the model's) of a checkpoint `fit` or the reference wrote
    -> (start_epoch, start_iterations) = (checkpoint["epoch"] + 1, checkpoint["iterations"]) for fit()."""
    stem.load_state_dict(checkpoint["state_dict"])
    optimizer.load_state_dict(checkpoint["optimizer"])
    aux_optimizer.load_state_dict(checkpoint["aux_optimizer"])
    lr_scheduler.load_state_dict(checkpoint["lr_scheduler"])
    return checkpoint["epoch"] + 1, checkpoint["iterations"]
