"""Save and resume a native training step: ``state_dict`` / ``load_state_dict`` of ``HRNetTrainStep`` and
``LifterTrainStep`` (one implementation, the step classes delegate here), and the way to and from
``torch.optim.Optimizer.state_dict()`` form.

The native steps own the optimizer's state: ``FlatParams`` holds the moments ``m`` / ``v`` and the device step counter,
``GroupedUpdate`` the AMSGrad maximum, the group table and the clip scalars, the lifter its dropout seed.  The torch
optimizer a caller hands to ``trainer.train`` is only read, so its ``state_dict()`` stays empty; what continues a run
is what this module writes.

A state dict holds plain containers and CPU tensors only (``torch.load(..., weights_only=True)`` reads it back), and it
is a snapshot: nothing in it aliases device memory or the step's host tables.  The parameters are not in it -- they are
the model's ``state_dict``.  Loading writes in place: ``flat``, ``m``, ``v``, ``vmax``, ``step_dev``, ``clip`` and the
device tables keep their addresses (captured graphs, ``StepCounters``' pointer table and the packed-filter caches hold
them), learning rates take the ``set_lrs`` / ``push_lrs`` route, and no later step launches anything it did not launch
before.  Nothing here launches a kernel of the library.

A ``GraphedStep`` keeps working when its step is loaded between two replays.  One limit: the lifter's dropout seed is a
kernel ARGUMENT, so a graph captured over a ``LifterTrainStep`` replays the seed it was captured with; load the state
before the capture when the masks matter."""
import torch

from . import optim as _optim

FORMAT = 1
_TORCH_CLASSES = {'adam': torch.optim.Adam, 'adamw': torch.optim.AdamW, 'sgd': torch.optim.SGD}
_EXTRAS = {'hrnet': ('apply_cr_loss',), 'lifter': ('drop_seed', '_noupdate_forwards')}
_PLAIN_KEYS = ('lr', 'betas', 'eps', 'momentum', 'weight_decay')      # the one set of the old entry points


def _names(step):
    return {id(p): name for name, p in step.model.named_parameters()}


def _plain_value(v):
    if isinstance(v, (tuple, list)):
        return [float(x) for x in v]
    return v if isinstance(v, bool) else float(v)


def optimizer_record(step):
    """family, the path ('grouped': the grouped update, else the old entry points), ``max_grad_norm`` and every
    group's hyper-parameters with its current learning rate and its parameters' names."""
    names = _names(step)
    if step.grouped is not None:
        rec = step.grouped.describe()
        groups = []
        for g in rec['groups']:
            row = {k: _plain_value(v) for k, v in g.items() if k != 'params'}
            row['params'] = [names[id(p)] for p in g['params'] if id(p) in names]
            groups.append(row)
        return {'family': rec['family'], 'grouped': True, 'max_grad_norm': rec['max_grad_norm'], 'groups': groups}
    row = {k: _plain_value(getattr(step, k)) for k in _PLAIN_KEYS}
    row['params'] = [names[id(p)] for p in step.flat.params]
    return {'family': step.optim_type, 'grouped': False, 'max_grad_norm': None, 'groups': [row]}


def state_dict(step):
    """The snapshot described in the module's doc string."""
    flat = step.flat
    state = flat.state()
    if step.grouped is not None:
        state.update(step.grouped.state())
    sd = {'format': FORMAT, 'kind': step.state_kind,
          'layout': {'numel': int(flat.numel), 'params': flat.layout(_names(step))},
          'optimizer': optimizer_record(step), 'state': state}
    for k in _EXTRAS[step.state_kind]:
        v = getattr(step, k)
        sd[k] = bool(v) if isinstance(v, bool) else int(v)
    return sd


def _check_layout(saved, mine):
    a, b = saved['params'], mine['params']
    for x, y in zip(a, b):
        if x['name'] != y['name']:
            raise ValueError('layout: saved parameter %r where this step has %r' % (x['name'], y['name']))
        if list(x['shape']) != list(y['shape']):
            raise ValueError('layout: parameter %r was saved with shape %s, this step has %s'
                             % (x['name'], tuple(x['shape']), tuple(y['shape'])))
        if int(x['offset']) != int(y['offset']):
            raise ValueError('layout: parameter %r was saved at offset %d, this step has it at %d'
                             % (x['name'], x['offset'], y['offset']))
    if len(a) != len(b):
        more, which = (a, 'the saved state') if len(a) > len(b) else (b, 'this step')
        raise ValueError('layout: %d parameters saved, this step has %d; %s has %r in addition'
                         % (len(a), len(b), which, more[min(len(a), len(b))]['name']))
    if int(saved['numel']) != int(mine['numel']):
        raise ValueError('layout: %d floats saved, this step has %d' % (saved['numel'], mine['numel']))


def _check_optimizer(saved, mine):
    if saved['family'] != mine['family']:
        raise ValueError('saved family %s, this step runs %s' % (saved['family'], mine['family']))
    if bool(saved['grouped']) != bool(mine['grouped']):
        which = lambda r: 'the grouped update' if r['grouped'] else 'the one-launch update'
        raise ValueError('saved by %s, this step runs %s' % (which(saved), which(mine)))
    if len(saved['groups']) != len(mine['groups']):
        raise ValueError('%d parameter groups saved, this step has %d' % (len(saved['groups']), len(mine['groups'])))
    for k, (x, y) in enumerate(zip(saved['groups'], mine['groups'])):
        if list(x['params']) != list(y['params']):
            diff = next((i for i, (p, q) in enumerate(zip(x['params'], y['params'])) if p != q),
                        min(len(x['params']), len(y['params'])))
            pick = lambda r: r['params'][diff] if diff < len(r['params']) else None
            raise ValueError('group %d: parameter %d was saved as %r, this step has %r' % (k, diff, pick(x), pick(y)))
        for key in sorted((set(x) | set(y)) - {'lr', 'params'}):
            if key not in x or key not in y or x[key] != y[key]:
                raise ValueError('group %d: %s was saved as %r, this step has %r' % (k, key, x.get(key), y.get(key)))
    if saved['max_grad_norm'] != mine['max_grad_norm']:
        raise ValueError('max_grad_norm was saved as %r, this step has %r'
                         % (saved['max_grad_norm'], mine['max_grad_norm']))


def load_state_dict(step, sd, strict=True):
    """Validate (``ValueError`` naming the first thing that differs), then write in place.  ``strict=False`` accepts a
    missing ``vmax`` or missing clip scalars and zeroes them; a different layout is never accepted."""
    if sd.get('format') != FORMAT:
        raise ValueError('training-state format %r (this version reads %d)' % (sd.get('format'), FORMAT))
    if sd['kind'] != step.state_kind:
        raise ValueError('saved by a %r step, this is a %r step' % (sd['kind'], step.state_kind))
    flat = step.flat
    _check_layout(sd['layout'], {'numel': flat.numel, 'params': flat.layout(_names(step))})
    _check_optimizer(sd['optimizer'], optimizer_record(step))
    state = sd['state']
    for k in ('m', 'v'):
        if tuple(state[k].shape) != (flat.numel,):
            raise ValueError('state %r holds %s floats, the layout %d' % (k, tuple(state[k].shape), flat.numel))
    more = {}
    if step.grouped is not None:
        for k, t in (('vmax', step.grouped.vmax), ('clip', step.grouped.clip)):
            if t is None:
                continue
            if state.get(k) is None:
                if strict:
                    raise ValueError('the saved state has no %r, this step keeps one (strict=False zeroes it)' % k)
            elif tuple(state[k].shape) != tuple(t.shape):
                raise ValueError('state %r has shape %s, this step %s' % (k, tuple(state[k].shape), tuple(t.shape)))
            more[k] = state.get(k)
    for k in _EXTRAS[step.state_kind]:
        if k not in sd:
            raise ValueError('the saved %s state has no %r' % (step.state_kind, k))
    # -- everything agrees: write ---------------------------------------------------------------------------------
    flat.load_state(state['m'], state['v'], int(state['step']))
    if step.grouped is not None:
        step.grouped.load_state(more.get('vmax'), more.get('clip'))
    step.set_lrs([g['lr'] for g in sd['optimizer']['groups']])
    for k in _EXTRAS[step.state_kind]:
        setattr(step, k, bool(sd[k]) if isinstance(getattr(step, k), bool) else int(sd[k]))
    from .engine import invalidate
    invalidate(step.model)                 # the model's weights usually came back with this state: re-fold them


# -- torch.optim.Optimizer.state_dict() form ---------------------------------------------------------------------------
def _family_rows(step):
    """(family, [row]): each row the family's torch hyper-parameters (every key of ``optim._DEFAULTS[family]``), the
    current ``lr`` and ``params``, the group's parameter tensors in the group's order."""
    if step.grouped is not None:
        rec = step.grouped.describe()
        return rec['family'], rec['groups']
    family = step.optim_type
    row = dict(_optim._DEFAULTS[family], lr=float(step.lr), weight_decay=float(step.weight_decay))
    if family == 'sgd':
        row['momentum'] = float(step.momentum)
    else:
        row.update(betas=(float(step.betas[0]), float(step.betas[1])), eps=float(step.eps))
    row['params'] = list(step.flat.params)
    return family, [row]


def _position(flat):
    return {id(p): i for i, p in enumerate(flat.params)}


def optimizer_state_dict(step):
    """The step's optimizer state as ``torch.optim.Adam`` / ``AdamW`` / ``SGD`` ``.state_dict()`` gives it, for an
    optimizer built over the step's groups: parameter indices count through the groups in order, as torch numbers
    them.  Per parameter ``step`` / ``exp_avg`` / ``exp_avg_sq`` (/ ``max_exp_avg_sq``), or ``momentum_buffer``: CPU
    copies of the parameter's own elements of the flat buffers, never the padding.  Before the first step (and for
    SGD without momentum) ``state`` is empty, as torch's is."""
    family, rows = _family_rows(step)
    flat, pos = step.flat, _position(step.flat)
    # the key set and the number format of the installed torch: an optimizer of its own over empty stand-ins
    shell = _TORCH_CLASSES[family]([dict({k: v for k, v in r.items() if k != 'params'},
                                         params=[torch.nn.Parameter(torch.empty(0)) for _ in r['params']])
                                    for r in rows])
    out = shell.state_dict()
    st = flat.state()
    t = st['step']
    vmax = step.grouped.state().get('vmax') if step.grouped is not None else None
    if t == 0 or (family == 'sgd' and not any(r['momentum'] for r in rows)):
        return out
    index = 0
    for r in rows:
        for p in r['params']:
            i = pos.get(id(p))
            if i is not None and not (family == 'sgd' and not r['momentum']):
                cut = lambda buf: flat.cut(buf, i).clone()
                if family == 'sgd':
                    out['state'][index] = {'momentum_buffer': cut(st['m'])}
                else:
                    ent = {'step': torch.tensor(float(t), dtype=torch.float32), 'exp_avg': cut(st['m']),
                           'exp_avg_sq': cut(st['v'])}
                    if r['amsgrad']:
                        ent['max_exp_avg_sq'] = cut(vmax)
                    out['state'][index] = ent
            index += 1
    return out


def _family_of_dict(groups, mine, family):
    if family is not None:
        return family
    g = groups[0]
    if 'betas' in g:
        if 'decoupled_weight_decay' in g:
            return 'adamw' if g['decoupled_weight_decay'] else 'adam'
        return mine if mine in ('adam', 'adamw') else 'adam'      # older dicts do not say which of the two
    return 'sgd' if 'momentum' in g else None


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(float(x) == float(y) for x, y in zip(a, b))
    return (bool(a) == bool(b)) if isinstance(a, bool) or isinstance(b, bool) else float(a) == float(b)


def load_optimizer_state_dict(step, torch_sd, family=None):
    """The inverse of ``optimizer_state_dict``: take over the state of a torch optimizer over the same groups.
    ``step`` may be an int, a float or a 0-d tensor and has to be the same for every parameter (the native update has
    one counter); family and per-group hyper-parameters have to agree with the step's, ``lr`` is taken from the dict;
    padding is zeroed; state for no parameter at all is the fresh optimizer (everything zero, counter 0), state for
    some but not all is refused.  ``family``: says which family wrote a dict that does not (Adam and AdamW dicts of
    older torch versions look alike).  SGD dicts carry no counter: with momentum buffers the counter becomes 1 unless
    the entries hold a ``step`` (the update only asks whether it is the first)."""
    mine, rows = _family_rows(step)
    groups, states = torch_sd['param_groups'], torch_sd['state']
    theirs = _family_of_dict(groups, mine, family)
    if theirs != mine:
        raise ValueError('the dict is of family %s, this step runs %s' % (theirs, mine))
    if len(groups) != len(rows):
        raise ValueError('%d param_groups in the dict, this step has %d' % (len(groups), len(rows)))
    names, flat, pos = _names(step), step.flat, _position(step.flat)
    for k, (g, r) in enumerate(zip(groups, rows)):
        if len(g['params']) != len(r['params']):
            raise ValueError('group %d: %d parameters in the dict, this step has %d'
                             % (k, len(g['params']), len(r['params'])))
        for key in r:
            if key in ('lr', 'params'):
                continue
            if key not in g or not _same(g[key], r[key]):
                raise ValueError('group %d: %s is %r in the dict, this step has %r' % (k, key, g.get(key), r[key]))
        if g.get('maximize', False):
            raise ValueError('group %d: maximize=True' % k)
    keys = {'m': 'momentum_buffer'} if mine == 'sgd' else {'m': 'exp_avg', 'v': 'exp_avg_sq', 'vmax': 'max_exp_avg_sq'}
    bufs = {k: torch.zeros(flat.numel, dtype=torch.float32) for k in keys}
    count, first, missing, found = None, None, None, None
    for g, r in zip(groups, rows):
        for idx, p in zip(g['params'], r['params']):
            i = pos.get(id(p))
            if i is None:
                continue                                   # a frozen parameter: torch keeps no state for it either
            name = names.get(id(p), 'parameter %d' % i)
            ent = states.get(idx)
            if not ent or (mine == 'sgd' and ent.get('momentum_buffer') is None):
                missing = missing or name
                continue
            found = found or name
            for k, tk in keys.items():
                if k == 'vmax' and not r['amsgrad']:
                    continue
                if ent.get(tk) is None:
                    raise ValueError('%r: the dict has no %s' % (name, tk))
                if tuple(ent[tk].shape) != tuple(p.shape):
                    raise ValueError('%r: %s has shape %s in the dict, the parameter %s'
                                     % (name, tk, tuple(ent[tk].shape), tuple(p.shape)))
                flat.cut(bufs[k], i).copy_(ent[tk].detach().to('cpu', torch.float32))
            if 'step' in ent:
                t = float(ent['step'])
                if t != int(t) or t < 0:
                    raise ValueError('%r: step %r is no iteration count' % (name, ent['step']))
                if count is None:
                    count, first = int(t), name
                elif int(t) != count:
                    raise ValueError('the native update has one step counter: %r is at step %d, %r at step %d'
                                     % (first, count, name, int(t)))
            elif mine != 'sgd':
                raise ValueError('%r: the dict has no step' % name)
    if found and missing:
        raise ValueError('the dict has state for %r and none for %r: all parameters or none' % (found, missing))
    if not found:
        count = 0
    elif count is None:
        count = 1                                          # SGD with momentum buffers: not the first step
    flat.load_state(bufs['m'], bufs.get('v'), count)
    if step.grouped is not None:
        step.grouped.load_state(bufs.get('vmax'), None)
    step.set_lrs([float(g['lr']) for g in groups])


# -- host random-number state in plain containers --------------------------------------------------------------------------
def rng_state(device=None):
    """Python's ``random``, numpy's global generator (``TrainSampleBuilder`` draws from it), torch's CPU generator and,
    for a CUDA ``device``, its generator -- tuples and arrays unpacked into lists, ints and floats."""
    import random
    import numpy as np
    version, words, gauss = random.getstate()
    kind, keys, position, has_gauss, cached = np.random.get_state()
    out = {'python': [int(version), [int(w) for w in words], gauss],
           'numpy': [str(kind), [int(k) for k in keys], int(position), int(has_gauss), float(cached)],
           'torch': torch.get_rng_state().clone(), 'cuda': None}
    if device is not None and torch.device(device).type == 'cuda':
        out['cuda'] = torch.cuda.get_rng_state(device).clone()
    return out


def set_rng_state(state, device=None):
    import random
    import numpy as np
    version, words, gauss = state['python']
    random.setstate((version, tuple(words), gauss))
    kind, keys, position, has_gauss, cached = state['numpy']
    np.random.set_state((kind, np.asarray(keys, dtype=np.uint32), position, has_gauss, cached))
    torch.set_rng_state(state['torch'].cpu())
    if state.get('cuda') is not None and device is not None and torch.device(device).type == 'cuda':
        torch.cuda.set_rng_state(state['cuda'].cpu(), device)
