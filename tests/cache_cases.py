"""Shared by tests/test_weight_caches.py (CPU) and tests/test_hip_weight_caches.py (GPU): the ways a parameter can change, a
never-run twin to compare against, and counters around the weight packers.

No kernel reads a `weight`: it reads a packed copy kept while a host-side key says the parameter has not changed
(layers._PackCache, engine.ensure_packed, EntropyModel.host_tables).  A MUTATION moves parameters by FACTOR in one of the ways a
user or this package writes them; the tests then require the next launch to see the new values.

  MUTATIONS        name -> fn(module, params): every way that torch's version counter, the tensor's address or the weight epoch sees
  STALE_MUTATION   the one way nobody sees (an in-place write through `.data`): documented behaviour, INTEGRATION.md
  make / twin      modules that remember their constructor arguments / a fresh copy loaded from the state dict
  count_packs      counters around every packer layers.py and engine.py look up
"""
import collections
import inspect

import torch

FACTOR = 1.5


def _moved(p):
    return p.detach().clone() * FACTOR


def inplace_no_grad(module, params):
    with torch.no_grad():
        for p in params:
            p.mul_(FACTOR)


def copy_from_new(module, params):
    with torch.no_grad():
        for p in params:
            p.copy_(_moved(p))


def _names(module, params):
    ids = {id(p): n for n, p in module.named_parameters()}
    return [ids[id(p)] for p in params]


def _moved_state(module, params):
    """a twin's state dict with the chosen parameters moved"""
    other = twin(module)
    sd = other.state_dict()
    with torch.no_grad():
        for n in _names(module, params):
            sd[n].mul_(FACTOR)
    return sd


def load_state_dict_(module, params):
    module.load_state_dict(_moved_state(module, params))


def load_state_dict_assign(module, params):
    """replaces the Parameter OBJECTS: callers must look the parameters up again afterwards"""
    module.load_state_dict(_moved_state(module, params), assign=True)


def _with_grads(params, step):
    """run `step` with .grad = -(FACTOR - 1) * p on the chosen parameters (SGD at lr 1 then multiplies them by FACTOR), and put
    the gradients back as they were (they may be views of a flat buffer)"""
    old = [p.grad for p in params]
    for p in params:
        p.grad = -(FACTOR - 1) * p.detach().clone()
    try:
        step()
    finally:
        for p, g in zip(params, old):
            p.grad = g


def _sgd(foreach):
    def mutate(module, params):
        _with_grads(params, torch.optim.SGD(params, lr=1.0, foreach=foreach).step)
    mutate.__name__ = f"sgd_foreach_{'on' if foreach else 'off'}"
    return mutate


def adam_step(module, params):
    # Adam's first step moves every element with a gradient by lr against the gradient's sign, whatever its size: away from zero
    # here, by about the size of a weight (elements that ARE zero, the masked taps, have no gradient and stay)
    lr = float(max(p.detach().abs().max() for p in params)) * (FACTOR - 1)
    _with_grads(params, torch.optim.Adam(params, lr=lr).step)


def rebind_data(module, params):
    for p in params:
        p.data = _moved(p)


def data_mul(module, params):
    """invisible to torch: neither the version counter nor the address moves"""
    for p in params:
        p.data.mul_(FACTOR)


def data_mul_bump_params(module, params):
    from spatiotemporalentropymodel_amd.layers import bump_weight_epoch
    data_mul(module, params)
    bump_weight_epoch(params)


def data_mul_bump_all(module, params):
    from spatiotemporalentropymodel_amd.layers import bump_weight_epoch
    data_mul(module, params)
    bump_weight_epoch()


def flat_of(module):
    """the FlatParameters over all of `module`'s parameters, made at the first request.  It re-homes them, which every key sees: a
    test of the two mutations below calls this BEFORE its warm run (`fn.prepare`), so that what the test sees is the write."""
    from spatiotemporalentropymodel_amd.optim import FlatParameters
    flat = getattr(module, "_cases_flat", None)
    if flat is None:
        flat = FlatParameters(sorted(module.named_parameters(), key=lambda t: t[0]))
        object.__setattr__(module, "_cases_flat", flat)
        for p in flat.params:
            p.grad = None                      # as after zero_grad(set_to_none=True): the layer-wise backward returns its gradients
    return flat


def fused_clip_adam_step(module, params):
    """FusedClipAdam.step over the module (GPU).  Parameters outside `params` have a zero gradient and zero moments: they stay bit for bit"""
    from spatiotemporalentropymodel_amd.optim import FusedClipAdam
    flat = flat_of(module)
    old = [p.grad for p in flat.params]
    flat.grad.zero_()
    for p in params:
        p._flat_grad_view.copy_(-p.detach())
    lr = float(max(p.detach().abs().max() for p in params)) * (FACTOR - 1)
    FusedClipAdam(flat, lr).step()
    flat.grad.zero_()
    for p, g in zip(flat.params, old):
        p.grad = g


def flat_restore(module, params):
    """a write into flat.data through FlatParameters.restore, the path graphs.GraphedPFrameStep puts a checkpoint back with"""
    flat = flat_of(module)
    data = flat.data.clone()
    for p in params:
        o = flat.offsets[[id(q) for q in flat.params].index(id(p))]
        data[o:o + p.numel()].mul_(FACTOR)
    flat.restore(data)


fused_clip_adam_step.prepare = flat_restore.prepare = flat_of
fused_clip_adam_step.gpu = True

_HAS_ASSIGN = "assign" in inspect.signature(torch.nn.Module.load_state_dict).parameters

MUTATIONS = collections.OrderedDict((f.__name__, f) for f in (
    [inplace_no_grad, copy_from_new, load_state_dict_] + ([load_state_dict_assign] if _HAS_ASSIGN else [])
    + [_sgd(True), _sgd(False), adam_step, rebind_data, data_mul_bump_params, data_mul_bump_all, fused_clip_adam_step, flat_restore]))
STALE_MUTATION = data_mul

#: the mutations a CPU test can run (FusedClipAdam.step is a HIP kernel)
CPU_MUTATIONS = collections.OrderedDict((n, f) for n, f in MUTATIONS.items() if not getattr(f, "gpu", False))


def prepare(mutation, module):
    """what `mutation` wants done before the warm run (nothing for most)"""
    hook = getattr(mutation, "prepare", None)
    if hook is not None:
        hook(module)


def lookup(module, names):
    """the parameters called `names` as they are NOW (load_state_dict(assign=True) replaces the objects)"""
    named = dict(module.named_parameters())
    return [named[n] for n in names]


# ----------------------------------------------------------------------------- twins
def make(cls, *args, **kwargs):
    """cls(*args, **kwargs), remembering the arguments for twin()"""
    m = cls(*args, **kwargs)
    object.__setattr__(m, "_cases_ctor", (cls, args, kwargs))
    return m


def _fresh(module):
    cls, args, kwargs = module._cases_ctor
    again = lambda a: _fresh(a) if isinstance(a, torch.nn.Module) else a
    return make(cls, *[again(a) for a in args], **{k: again(v) for k, v in kwargs.items()})


def twin(module):
    """A freshly constructed module of the same class and arguments (`module` comes from make(); so do module arguments such as
    the children of a FusedSequential), on the same device and in the same mode, loaded from module.state_dict().  It has never
    run: cold caches, same plan, same kernels."""
    other = _fresh(module)
    p = next(iter(module.parameters()), None)
    if p is not None:
        other = other.to(p.device)
    other.load_state_dict(module.state_dict())
    other.train(module.training)
    return other


# ----------------------------------------------------------------------------- pack counters
class PackCounts(collections.Counter):
    """name -> calls; `.weights[name]`: the data_ptr of the tensor each call packed (first argument)"""

    def __init__(self):
        super().__init__()
        self.weights = collections.defaultdict(list)

    def reset(self):
        self.clear()
        self.weights.clear()

    def total(self):
        return sum(self.values())


def count_packs(monkeypatch):
    """Wrap the packers where layers.py and engine.py look them up: the layers._PACKERS entries (counted under the role's name) and
    F.pack_weight / c4gdn_stream / pack_weights_multi / pack_weights_f16x2_multi / pack_weights_f16x2_pair_multi.  -> PackCounts"""
    from spatiotemporalentropymodel_amd import functional as F
    from spatiotemporalentropymodel_amd import layers
    counts = PackCounts()

    def counted(name, fn):
        def wrapper(*args, **kwargs):
            counts[name] += 1
            if args and isinstance(args[0], torch.Tensor):
                counts.weights[name].append(args[0].data_ptr())
            return fn(*args, **kwargs)
        return wrapper

    role_names = {getattr(layers, n): n for n in dir(layers) if n.startswith("PACK_") and isinstance(getattr(layers, n), int)}
    for role, fn in list(layers._PACKERS.items()):
        monkeypatch.setitem(layers._PACKERS, role, counted(role_names[role], fn))
    for name in ("pack_weight", "c4gdn_stream", "pack_weights_multi", "pack_weights_f16x2_multi", "pack_weights_f16x2_pair_multi"):
        monkeypatch.setattr(F, name, counted(name, getattr(F, name)))
    return counts
