"""The native optimizer step for parameter groups (csrc/optim.hip): ``torch.optim.Adam`` / ``AdamW`` / ``SGD`` with any
number of ``param_groups``, AMSGrad, Nesterov, dampening, and ``torch.nn.utils.clip_grad_norm_`` (norm_type 2) folded
into the update -- one update launch over the flat parameter buffer whatever the number of groups.

This module owns the spec, the tables and every call of the entry points ``egn_optim_grouped_step_f32`` and
``egn_grad_norm_clip_f32``; the step modules call ``GroupedUpdate``'s methods.  What the three old entry points can
express (one set of hyper-parameters, Adam or SGD, no AMSGrad / Nesterov / dampening, no clipping) never comes here:
``plain_kwargs`` hands it back to ``FlatParams.update``, with the launches and the bits it always had.

Departure from torch, on purpose: ``clip_grad_norm_`` scales ``p.grad`` in place; here the coefficient is multiplied
in as the update loads the gradient, so ``p.grad`` keeps its unclipped values after the step (no extra pass over the
gradient).  There is no torch fall-back."""
import numpy as np
import torch

from . import _lib

FAMILIES = {'adam': 0, 'adamw': 1, 'sgd': 2}
AMSGRAD, NESTEROV = 1, 2
MAX_GROUPS = 32
GROUP_DTYPE = np.dtype([('lr', '<f4'), ('weight_decay', '<f4'), ('beta1', '<f4'), ('beta2', '<f4'), ('eps', '<f4'),
                        ('momentum', '<f4'), ('dampening', '<f4'), ('flags', '<i4')])
ITEM_DTYPE = np.dtype([('begin', '<i8'), ('length', '<i4'), ('group', '<i4')])

_DEFAULTS = {
    'adam': dict(lr=1e-3, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, amsgrad=False),
    'adamw': dict(lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8, amsgrad=False),
    'sgd': dict(lr=1e-3, weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=False),
}


class Spec(object):
    """family ('adam' / 'adamw' / 'sgd') and the groups: dicts of params (a list of tensors) and the family's
    hyper-parameters, every key present."""

    def __init__(self, family, groups):
        self.family, self.groups = family, groups

    @property
    def lrs(self):
        return [g['lr'] for g in self.groups]


def spec(family, groups, **defaults):
    """``spec('adamw', [dict(params=[...], lr=1e-4), dict(params=[...], weight_decay=0.0)], lr=1e-3)``: per-group keys
    over ``defaults`` over torch's own defaults of the family."""
    if family not in FAMILIES:
        raise NotImplementedError('optimizer family %r (adam, adamw, sgd)' % (family,))
    base = dict(_DEFAULTS[family])
    unknown = sorted(set(defaults) - set(base))
    if unknown:
        raise TypeError('%s has no hyper-parameter %s' % (family, ', '.join(unknown)))
    base.update(defaults)
    if not groups:
        raise ValueError('an optimizer spec needs at least one group')
    if len(groups) > MAX_GROUPS:
        raise NotImplementedError('%d parameter groups (the group table holds %d)' % (len(groups), MAX_GROUPS))
    out, seen = [], set()
    for g in groups:
        g = dict(g)
        unknown = sorted(set(g) - set(base) - {'params'})
        if unknown:
            raise TypeError('%s group has no key %s' % (family, ', '.join(unknown)))
        params = g.get('params')
        params = [params] if torch.is_tensor(params) else list(params or ())
        for p in params:
            if id(p) in seen:
                raise ValueError('a parameter appears in more than one group')
            seen.add(id(p))
        row = dict(base)
        row.update(g)
        row['params'] = params
        if torch.is_tensor(row['lr']):
            raise NotImplementedError('a tensor lr (the table holds host floats the scheduler rewrites)')
        for k in row:
            if k == 'betas':
                row[k] = (float(row[k][0]), float(row[k][1]))
            elif k in ('amsgrad', 'nesterov'):
                row[k] = bool(row[k])
            elif k != 'params':
                row[k] = float(row[k])
        _check_group(family, row)
        out.append(row)
    return Spec(family, out)


def _check_group(family, g):
    """torch's own constructor rules (the library checks them again on the table)."""
    if g['lr'] < 0 or g['weight_decay'] < 0:
        raise ValueError('negative lr / weight_decay')
    if family == 'sgd':
        if g['momentum'] < 0 or not 0.0 <= g['dampening'] <= 1.0:
            raise ValueError('momentum must be >= 0 and dampening within [0, 1]')
        if g['nesterov'] and (g['momentum'] <= 0 or g['dampening'] != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
    else:
        if not (0.0 <= g['betas'][0] < 1.0 and 0.0 <= g['betas'][1] < 1.0) or g['eps'] <= 0:
            raise ValueError('betas must lie in [0, 1) and eps be positive')


def _family_of(optimizer):
    if isinstance(optimizer, torch.optim.AdamW):
        return 'adamw'
    if type(optimizer) is torch.optim.Adam:
        return 'adam'
    if type(optimizer) is torch.optim.SGD:
        return 'sgd'
    raise NotImplementedError('native update for %s (Adam, AdamW, SGD)' % type(optimizer).__name__)


def spec_from_torch(optimizer):
    """The spec of a ``torch.optim.Adam`` / ``AdamW`` / ``SGD`` object, every group's ``lr`` honoured.  ``foreach`` /
    ``fused`` / ``capturable`` / ``differentiable`` do not change the arithmetic and are ignored."""
    family = _family_of(optimizer)
    groups = []
    for g in optimizer.param_groups:
        if g.get('maximize', False):
            raise NotImplementedError('%s(maximize=True)' % type(optimizer).__name__)
        if torch.is_tensor(g['lr']):
            raise NotImplementedError('%s with a tensor lr' % type(optimizer).__name__)
        if g.get('decoupled_weight_decay', False) and family == 'adam':
            family = 'adamw'
        groups.append({k: g[k] for k in list(_DEFAULTS[family]) + ['params'] if k in g})
    return spec(family, groups)


def plain_kwargs(sp, max_grad_norm=None):
    """The keywords of the old one-launch update (lr, optim_type, betas, eps, momentum, weight_decay) where the three
    old entry points can express ``sp`` -- one set of hyper-parameters, Adam or SGD, no AMSGrad / Nesterov / dampening,
    no clipping -- else None."""
    if max_grad_norm is not None or sp.family == 'adamw':
        return None
    g0 = sp.groups[0]
    keys = [k for k in g0 if k != 'params']
    if any(g[k] != g0[k] for g in sp.groups[1:] for k in keys):
        return None
    if sp.family == 'sgd':
        if g0['nesterov'] or g0['dampening']:
            return None
        return dict(lr=g0['lr'], optim_type='sgd', momentum=g0['momentum'], weight_decay=g0['weight_decay'])
    if g0['amsgrad']:
        return None
    return dict(lr=g0['lr'], optim_type='adam', betas=g0['betas'], eps=g0['eps'], weight_decay=g0['weight_decay'])


def needs_grouped(optimizer, max_grad_norm=None):
    """Whether ``trainer.make_step`` has to hand the torch optimizer over as a spec: differing groups (differing
    ``lr`` included), AdamW, AMSGrad, Nesterov, dampening or clipping.  Raises for what no path takes."""
    return plain_kwargs(spec_from_torch(optimizer), max_grad_norm) is None


def step_spec(o, optim_spec, max_grad_norm):
    """For a step object's constructor: the spec the grouped path runs, or None for the old path -- after writing an
    expressible spec's hyper-parameters onto ``o`` (lr, optim_type, betas, eps, momentum, weight_decay)."""
    if optim_spec is None and max_grad_norm is None:
        return None
    if optim_spec is None:
        if o.optim_type == 'sgd':
            optim_spec = spec('sgd', [dict(params=list(o.model.parameters()))], lr=o.lr, momentum=o.momentum,
                              weight_decay=o.weight_decay)
        else:
            optim_spec = spec('adam', [dict(params=list(o.model.parameters()))], lr=o.lr, betas=o.betas, eps=o.eps,
                              weight_decay=o.weight_decay)
    plain = plain_kwargs(optim_spec, max_grad_norm)
    if plain is None:
        o.lr = optim_spec.groups[0]['lr']
        return optim_spec
    for k, val in plain.items():
        setattr(o, k, val)
    return None


# -- the tables ---------------------------------------------------------------------------------------------------
def group_table(sp):
    """numpy [ngroups] of GROUP_DTYPE (egn_optim_group)."""
    t = np.zeros(len(sp.groups), dtype=GROUP_DTYPE)
    for k, g in enumerate(sp.groups):
        if sp.family == 'sgd':
            t[k] = (g['lr'], g['weight_decay'], 0.0, 0.0, 0.0, g['momentum'], g['dampening'],
                    NESTEROV if g['nesterov'] else 0)
        else:
            t[k] = (g['lr'], g['weight_decay'], g['betas'][0], g['betas'][1], g['eps'], 0.0, 0.0,
                    AMSGRAD if g['amsgrad'] else 0)
    return t


def segments(params, offsets, numel, sp):
    """[(begin, end, group)] in floats of the flat buffer: maximal runs of one group, a parameter's padding with the
    parameter.  A trainable parameter that is in no group is a ValueError, as is a group's parameter that is not in
    the buffer."""
    owner = {id(p): k for k, g in enumerate(sp.groups) for p in g['params']}
    flat_ids = {id(p) for p in params}
    stray = [k for k, g in enumerate(sp.groups) for p in g['params'] if id(p) not in flat_ids and p.requires_grad]
    if stray:
        raise ValueError('group %d holds a trainable parameter that is not the model\'s' % stray[0])
    segs = []
    for i, p in enumerate(params):
        if id(p) not in owner:
            raise ValueError('trainable parameter %d (shape %s) is in no parameter group' % (i, tuple(p.shape)))
        end = offsets[i + 1] if i + 1 < len(params) else numel
        if segs and segs[-1][2] == owner[id(p)]:
            segs[-1] = (segs[-1][0], end, segs[-1][2])
        else:
            segs.append((offsets[i], end, owner[id(p)]))
    return segs


def work_items(segs, item_floats):
    """numpy [nitems] of ITEM_DTYPE (egn_optim_item): every segment cut into items of at most ``item_floats`` floats.
    Items never cross a segment boundary and cover the buffer exactly once, in order."""
    begins, lengths, groups = [], [], []
    for b, e, k in segs:
        if b % 4 or e % 4 or e <= b:
            raise ValueError('segment [%d, %d) is not a run of whole float4' % (b, e))
        bs = np.arange(b, e, item_floats, dtype=np.int64)
        begins.append(bs)
        lengths.append(np.minimum(e - bs, item_floats).astype(np.int32))
        groups.append(np.full(len(bs), k, dtype=np.int32))
    t = np.zeros(sum(len(b) for b in begins), dtype=ITEM_DTYPE)
    t['begin'], t['length'], t['group'] = np.concatenate(begins), np.concatenate(lengths), np.concatenate(groups)
    return t


def _to_device(table, dev):
    return torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev)


def grouped_step(family, p, g, m, v, vmax, n, groups_host, groups_dev, items_host, items_dev, clip, step_dev, stream):
    """egn_optim_grouped_step_f32 on tensors (None -> NULL) and the host / device copies of the two tables; returns
    the library's code."""
    return _lib.lib().egn_optim_grouped_step_f32(
        FAMILIES[family], _lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), _lib.ptr(vmax), n,
        groups_host.ctypes.data, _lib.ptr(groups_dev), len(groups_host), items_host.ctypes.data, _lib.ptr(items_dev),
        len(items_host), _lib.ptr(clip), _lib.ptr(step_dev), stream)


def grad_norm_clip(g, n, max_norm, ws, clip, stream):
    """egn_grad_norm_clip_f32: clip[0] = total_norm, clip[1] = the coefficient; returns the library's code."""
    return _lib.lib().egn_grad_norm_clip_f32(_lib.ptr(g), n, max_norm, _lib.ptr(ws), _lib.ptr(clip), stream)


def norm_workspace(dev):
    return torch.empty(_lib.lib().egn_grad_norm_ws_bytes() // 8, dtype=torch.float64, device=dev)


class GroupedUpdate(object):
    """The grouped update of one step object: the tables on the host and on the device, the AMSGrad buffer where a
    group asks for it, the clip scalars.  ``flat``: the step's ``FlatParams`` (``m`` is SGD's momentum buffer)."""

    def __init__(self, flat, sp, max_grad_norm=None):
        dev = flat.flat.device
        self.flat, self.spec, self.family = flat, sp, sp.family
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if self.max_grad_norm is not None and not self.max_grad_norm >= 0:
            raise ValueError('max_grad_norm must be >= 0, got %r' % (max_grad_norm,))
        self.groups_host = group_table(sp)
        self.segments = segments(flat.params, flat.offsets, flat.numel, sp)
        self.items_host = work_items(self.segments, _lib.lib().egn_optim_item_floats())
        self.groups_dev = _to_device(self.groups_host, dev)
        self.items_dev = _to_device(self.items_host, dev)
        self.vmax = torch.zeros_like(flat.flat) if sp.family != 'sgd' and any(g['amsgrad'] for g in sp.groups) else None
        self.clip = self.norm_ws = None
        if self.max_grad_norm is not None:
            self.clip = torch.zeros(2, dtype=torch.float32, device=dev)
            self.norm_ws = norm_workspace(dev)
        self._dirty = False
        self.host_lrs = [g['lr'] for g in sp.groups]      # as given (the table holds them rounded to float32)

    # -- save / resume (train_state.py): this object's part -----------------------------------------------------
    def describe(self):
        """family, ``max_grad_norm`` and the groups: the spec's rows (``params`` the tensors) with the current
        learning rates."""
        return {'family': self.family, 'max_grad_norm': self.max_grad_norm,
                'groups': [dict(g, lr=lr) for g, lr in zip(self.spec.groups, self.host_lrs)]}

    def state(self):
        """CPU copies of ``vmax`` and the clip scalars, each where it exists."""
        return {k: t.detach().to('cpu', copy=True) for k, t in (('vmax', self.vmax), ('clip', self.clip))
                if t is not None}

    def load_state(self, vmax, clip):
        """In place; None zeroes.  The tables are not touched: learning rates come through ``set_lrs``."""
        with torch.no_grad():
            for t, src in ((self.vmax, vmax), (self.clip, clip)):
                if t is not None:
                    t.zero_() if src is None else t.copy_(src)

    @property
    def lrs(self):
        return [float(x) for x in self.groups_host['lr']]

    @property
    def last_grad_norm(self):
        """The device scalar ``total_norm`` of the last step (None without clipping); nothing is read back."""
        return None if self.clip is None else self.clip[0]

    def set_lrs(self, lrs):
        """One learning rate per group, as the scheduler left them; the device table is refilled by ``push_lrs`` only
        when a value has changed."""
        lrs = [float(x) for x in lrs]
        if len(lrs) != len(self.groups_host):
            raise ValueError('%d learning rates for %d parameter groups' % (len(lrs), len(self.groups_host)))
        new = np.asarray(lrs, dtype=np.float32)
        if not np.array_equal(new, self.groups_host['lr']):
            if not np.all(np.isfinite(new)) or np.any(new < 0):
                raise ValueError('learning rates must be finite and >= 0: %r' % (lrs,))
            self.groups_host['lr'] = new
            self._dirty = True
        self.host_lrs = lrs

    def push_lrs(self):
        """Refill the device table if ``set_lrs`` changed it (never inside a graph: ``GraphedStep`` calls this before
        each replay, an eager step at its update)."""
        if self._dirty:
            self.groups_dev.copy_(_to_device(self.groups_host, 'cpu'))
            self._dirty = False

    def state_tensors(self):
        """What a step mutates beyond FlatParams' own buffers (``GraphedStep`` restores it after its warm-up)."""
        return [t for t in (self.vmax, self.clip) if t is not None]

    def update(self, stream):
        f = self.flat
        if self._dirty and not torch.cuda.is_current_stream_capturing():
            self.push_lrs()
        if self.clip is not None:
            _lib.check(grad_norm_clip(f.grad, f.numel, self.max_grad_norm, self.norm_ws, self.clip, stream),
                       'gradient norm')
        _lib.check(grouped_step(self.family, f.flat, f.grad, f.m, f.v, self.vmax, f.numel, self.groups_host,
                                self.groups_dev, self.items_host, self.items_dev, self.clip, f.step_dev, stream),
                   'grouped optimizer step')


def attach(o, optim_spec, max_grad_norm):
    """For a step object's constructor, after ``o.flat`` exists: ``o.grouped`` = the grouped update or None."""
    if optim_spec is not None:            # whichever path runs it: every trainable parameter is in a group
        segments(o.flat.params, o.flat.offsets, o.flat.numel, optim_spec)
    sp = step_spec(o, optim_spec, max_grad_norm)
    o.grouped = None if sp is None else GroupedUpdate(o.flat, sp, max_grad_norm)
    o.max_grad_norm = max_grad_norm if o.grouped is not None else None


def set_lrs(o, lrs):
    """``step.set_lrs``: every group's learning rate (the old path has one: the first)."""
    lrs = list(lrs)
    if o.grouped is not None:
        o.grouped.set_lrs(lrs)
    elif len(set(lrs)) > 1:
        raise ValueError('this step has one learning rate; got %r' % (lrs,))
    o.lr = lrs[0]


def no_decay_groups(model, weight_decay, **kw):
    """The common split: conv / linear weights keep ``weight_decay``; BatchNorm (and every other normalisation's)
    gamma / beta and all biases get 0.  Returns the two group dicts for ``spec`` or a torch optimizer."""
    decay, rest = [], []
    norms = (torch.nn.modules.batchnorm._NormBase, torch.nn.GroupNorm, torch.nn.LayerNorm)
    for mod in model.modules():
        for name, p in mod.named_parameters(recurse=False):
            if not p.requires_grad:
                continue
            (rest if isinstance(mod, norms) or name.endswith('bias') or p.ndim <= 1 else decay).append(p)
    return [dict(params=decay, weight_decay=float(weight_decay), **kw), dict(params=rest, weight_decay=0.0, **kw)]
