"""CPU: the cadence of trainer.fit (the epoch loop of stem/trainSTEM.py:172-262) on stand-ins for the trainer, the loaders and the
scheduler: when the validation pass fires, what is checkpointed under which name, and how a run resumes."""
import os

import torch

from spatiotemporalentropymodel_amd import trainer as T


class _State:
    def __init__(self, **kv):
        self.kv = dict(kv)

    def state_dict(self):
        return dict(self.kv)

    def load_state_dict(self, d):
        self.kv = dict(d)


class _Scheduler(_State):
    def __init__(self):
        super().__init__(num_bad_epochs=0)
        self.seen = []

    def step(self, loss):
        self.seen.append(loss)
        self.kv["num_bad_epochs"] += 1


class _Trainer:
    """train_septuplet runs len(images) - 1 "P-frame steps" and calls on_step after each, as SeptupletTrainer does; validate returns
    the next of `losses` and steps the scheduler with it, as trainer.validate does"""

    def __init__(self, losses):
        self.stem, self.opt, self.aux_opt = _State(w=0), _State(t=0), _State(t=0)
        self.on_step = None
        self.losses = list(losses)
        self.events = []              # ("step", global step index, position in the septuplet) | ("val", steps so far, learning-rate epoch)
        self.steps = 0
        self.finished = 0

    def train_septuplet(self, images):
        for t in range(1, len(images)):
            self.steps += 1
            self.stem.kv["w"] = self.steps
            self.events.append(("step", self.steps, t))
            if self.on_step is not None:
                self.on_step(t, None, None, None, None)

    def validate(self, loader, lr_scheduler=None):
        assert loader == "TEST"
        loss = self.losses.pop(0)
        self.events.append(("val", self.steps))
        if lr_scheduler is not None:
            lr_scheduler.step(loss)
        return {"loss": loss, "y_bpp_loss": loss, "z_bpp_loss": 0.0, "count": 1.0}

    def finish(self):
        self.finished += 1


# the four subsamplings of stem/trainSTEM.py:175-182 leave 2, 3, 4 or 7 frames: 1, 2, 3 or 6 P-frame steps
LOADER = [[0] * 4, [0] * 2, [0] * 7, [0] * 3, [0] * 7, [0] * 2]          # 3 + 1 + 6 + 2 + 6 + 1 = 19 steps per epoch


def test_validation_fires_on_the_iterations_the_reference_counts(tmp_path):
    tr, sch = _Trainer([5.0, 4.0, 4.5, 3.0, 3.5, 9.0, 9.0]), _Scheduler()
    seen = []
    user = []
    tr.on_step = lambda t, *rest: user.append(t)
    res = T.fit(tr, LOADER, "TEST", sch, epochs=2, validate_every=7, save=None,
                on_validation=lambda epoch, it, r, best: seen.append((epoch, it, r["loss"], best)))
    # `iterations` counts P-frame steps across items and epochs (:226); the pass runs right after the step that makes it a multiple
    assert res["iterations"] == 38 and tr.steps == 38
    vals = [e[1] for e in tr.events if e[0] == "val"]
    assert vals == [7, 14, 21, 28, 35]
    # ... in the middle of a septuplet: step 7 is the third of item 2's six steps, and step 8 (its fourth) follows the pass
    i7 = tr.events.index(("val", 7))
    assert tr.events[i7 - 1] == ("step", 7, 3) and tr.events[i7 + 1] == ("step", 8, 4)
    i14 = tr.events.index(("val", 14))
    assert tr.events[i14 - 1] == ("step", 14, 2) and tr.events[i14 + 1] == ("step", 15, 3)
    assert seen == [(0, 7, 5.0, True), (0, 14, 4.0, True), (1, 21, 4.5, False), (1, 28, 3.0, True), (1, 35, 3.5, False)]
    assert sch.seen == [5.0, 4.0, 4.5, 3.0, 3.5]
    assert res["best_loss"] == 3.0 and res["validations"] == [(0, 7, 5.0), (0, 14, 4.0), (1, 21, 4.5), (1, 28, 3.0), (1, 35, 3.5)]
    # the caller's own hook still ran after every step and is back in place
    assert len(user) == 38 and tr.on_step is not None and tr.on_step.__name__ == "<lambda>"
    assert not os.listdir(tmp_path)


def test_validate_every_one_and_never():
    tr, sch = _Trainer([1.0] * 19), _Scheduler()
    T.fit(tr, LOADER, "TEST", sch, epochs=1, validate_every=1)
    assert [e[0] for e in tr.events] == ["step", "val"] * 19
    tr = _Trainer([])
    assert T.fit(tr, LOADER, "TEST", sch, epochs=1, validate_every=10 ** 9)["validations"] == []


def test_checkpoints_carry_the_references_keys_and_names(tmp_path):
    tr, sch = _Trainer([5.0, 6.0, 4.0, 7.0, 7.0, 7.0]), _Scheduler()
    prefix = str(tmp_path) + os.sep + "run_"
    T.fit(tr, LOADER, "TEST", sch, epochs=3, validate_every=10, save=prefix)
    names = sorted(os.listdir(tmp_path))
    # best-loss checkpoints at iterations 10 (epoch 0, 5.0) and 30 (epoch 1, 4.0) -- 6.0 at 20 is no improvement --; the periodic ones
    # after epochs 0 and 2 (:250 `epoch % 2 == 0`)
    assert names == ["run_checkpoint_best_epoch0.pth.tar", "run_checkpoint_best_epoch1.pth.tar", "run_checkpoint_epoch0.pth.tar",
                     "run_checkpoint_epoch2.pth.tar"]
    keys = {"epoch", "iterations", "state_dict", "optimizer", "aux_optimizer", "lr_scheduler"}
    best1 = torch.load(prefix + "checkpoint_best_epoch1.pth.tar", weights_only=False)
    assert set(best1) == keys and best1["epoch"] == 1 and best1["iterations"] == 30 and best1["state_dict"] == {"w": 30}
    assert best1["lr_scheduler"] == {"num_bad_epochs": 3}              # written after lr_scheduler.step(eval_loss), as :231-245
    ep0 = torch.load(prefix + "checkpoint_epoch0.pth.tar", weights_only=False)
    assert set(ep0) == keys and ep0["epoch"] == 0 and ep0["iterations"] == 19 and ep0["state_dict"] == {"w": 19}
    assert tr.finished >= 4                                            # the step's auxiliary stream is joined before a state is read


def test_resuming_continues_epoch_and_iterations(tmp_path):
    prefix = str(tmp_path) + os.sep
    tr, sch = _Trainer([5.0] * 9), _Scheduler()
    T.fit(tr, LOADER, "TEST", sch, epochs=1, validate_every=10, save=prefix)
    ck = torch.load(prefix + "checkpoint_epoch0.pth.tar", weights_only=False)
    tr2, sch2 = _Trainer([4.0, 3.0, 6.0, 6.0]), _Scheduler()
    start_epoch, start_it = T.resume_state(ck, tr2.stem, tr2.opt, tr2.aux_opt, sch2)
    assert (start_epoch, start_it) == (1, 19) and tr2.stem.kv == {"w": 19} and sch2.kv == {"num_bad_epochs": 1}
    seen = []
    res = T.fit(tr2, LOADER, "TEST", sch2, epochs=3, start_epoch=start_epoch, start_iterations=start_it, validate_every=10, save=prefix,
                on_validation=lambda epoch, it, r, best: seen.append((epoch, it)))
    # iterations 20 .. 38 are the resumed run's epoch 1, 39 .. 57 its epoch 2: the passes at 20, 30, 40 and 50 follow its steps 1, 11, 21, 31
    assert seen == [(1, 20), (1, 30), (2, 40), (2, 50)] and res["iterations"] == 19 + 38
    assert [e[1] for e in tr2.events if e[0] == "val"] == [1, 11, 21, 31]
    assert os.path.exists(prefix + "checkpoint_epoch2.pth.tar") and not os.path.exists(prefix + "checkpoint_epoch1.pth.tar")
    assert torch.load(prefix + "checkpoint_epoch2.pth.tar", weights_only=False)["epoch"] == 2
