"""Every call rl_agents_amd/native.py makes into the library, pinned against a recorded run (host only, no library).

A recording stand-in takes the place of libmi355plan.so: each call is checked against the symbol's SIGNATURES argtypes,
recorded with its addresses resolved to the arrays they point at (dtype, shape, content at call time), and answered by
writing a pattern that depends on the argument's position into every array and by filling the byref outputs.  What the
method returns, the caller's generator records after the call and any exception are recorded with it.  The record of
every case must equal tests/binding_calls.json, which ``python tests/test_binding_calls_host.py --write`` writes.
"""
import ctypes as C
import functools
import hashlib
import json
import os
import sys
import warnings

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # (after PYTHONPATH: it chooses the native.py)

from rl_agents_amd import native  # noqa: E402

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "binding_calls.json")
A, S, M, HORIZON = 3, 10, 2, 4
SIZES = (1, 2, 65)
CTX_H, MODEL_H, POLICY_H, RNG_H, PLANNERS_H, DEVICE_RNG_PTR, STREAM = 0xC0, 0xD0, 0xE0, 0xF0, 0x1A0, 0x7AB000, 0x5EED
SCALARS = (C.c_int, C.c_int32, C.c_int64, C.c_double)
BYREF_VALUES = {"mp_saopd_info": (2, 6, 2, S), "mp_gbopd_info": (2, S, A, 4, 6), "mp_gbop_info": (2, S, A, 2, 4, 6, 9),
                "mp_uct_tree_capacity": (7,),
                "mp_uct_stoch_tree_capacity": (7,), "mp_ctx_device_faults": (3,)}
NAMES = b"form_a form_b"


def _content(a):
    a = np.ascontiguousarray(a)
    if a.size <= 12:
        return a.reshape(-1).tolist()
    return "sha1:" + hashlib.sha1(a.tobytes()).hexdigest()[:16]


def _array(a):
    return ["array", str(a.dtype), list(a.shape), _content(a)]


class Lib(object):
    """The recording stand-in of the library."""

    def __init__(self):
        self.calls, self.seen, self.blocks, self.pinned = [], [], [], []
        self.returns, self.hooks, self.handles, self.ctx = {}, {}, 0, None

    def remember(self, a):
        if hasattr(a, "data_ptr"):
            self.seen.append(a.numpy())
        elif isinstance(a, np.ndarray):
            self.seen.append(a)
        return a

    def __getattr__(self, name):
        if name not in native.SIGNATURES:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _resolve(self, addr):
        for a in reversed(self.seen):
            if a.size and a.ctypes.data == addr:
                return a
        for p in self.pinned + list(self.ctx.__dict__.get("_pin_cache", {}).values()):
            for a in p.values():
                if a.size and a.ctypes.data == addr:
                    return a
        return None

    def _pointer(self, a, i, outs):
        if a is None:
            return ["null"]
        if isinstance(a, C.c_void_p):
            return ["pinned_block"] if any(a.value == C.addressof(b) for b in self.blocks) else ["c_void_p", a.value]
        if hasattr(a, "_obj"):                              # byref(...)
            outs.append((i, a._obj))
            return ["byref", type(a._obj).__name__]
        if isinstance(a, C.Array):
            if a._type_ is C.c_void_p:
                return ["pointers", [self._pointer(v, i, outs) for v in a]]
            return ["c_array", a._type_.__name__, list(a)]
        if a == DEVICE_RNG_PTR:
            return ["device_rng"]
        arr = self._resolve(a)
        if arr is None:
            return ["unresolved"]
        outs.append((i, arr))
        return _array(arr)

    def _call(self, name, args):
        restype, argtypes = native.SIGNATURES[name]
        assert len(args) == len(argtypes), "{}: {} arguments for {}".format(name, len(args), len(argtypes))
        rec, outs = [], []
        for i, (t, a) in enumerate(zip(argtypes, args)):
            t.from_param(a)                                 # what ctypes itself would refuse raises here
            if t in SCALARS:
                rec.append([t.__name__, t(a).value])
            elif t is C.c_char_p:
                rec.append(["buffer"])
            else:
                rec.append(self._pointer(a, i, outs))
        if name == "mp_model_load_cartpole":
            cp = native.CartPoleParams.from_address(args[1])
            rec[1] = ["cartpole", [getattr(cp, k) for k, _ in native.CartPoleParams._fields_]]
        self.calls.append([name, rec])
        refs = iter(BYREF_VALUES.get(name, ()))
        for i, o in outs:
            if isinstance(o, np.ndarray):
                if o.flags.writeable:
                    o.reshape(-1)[:] = (i * 1000 + np.arange(o.size) + (0.5 if o.dtype.kind == "f" else 0)).astype(o.dtype)
            elif isinstance(o, C.c_void_p):
                if name == "mp_host_alloc":
                    self.blocks.append((C.c_uint8 * args[1])())
                    o.value = C.addressof(self.blocks[-1])
                else:
                    self.handles += 1
                    o.value = 0x200 + 0x10 * self.handles
            elif isinstance(o, C.c_char_p):
                o.value = b"uct_form"
            elif isinstance(o, C.c_double):
                o.value = 1.5
            elif name.endswith("_export") and i == 3:       # the node count: fewer than cap (6 for a sizing call)
                o.value = 6 if args[2] == 0 else max(args[2] - 2, 1)
            else:
                o.value = next(refs, 5)
        if name in self.hooks:
            self.hooks[name](*[o for _, o in outs])
        if name in self.returns:
            return self.returns[name]
        if restype is C.c_char_p:
            return b"boom" if name == "mp_last_error" else NAMES
        if name == "mp_rng_device_ptr":
            return DEVICE_RNG_PTR
        return {"mp_abi_version": 7, "mp_libm_sincos_variant": 1, "mp_vi_graph_captures": 3}.get(name, 0)


class _Numpy(object):
    """numpy as native.py sees it: the arrays it makes are remembered, so that an address taken without _ptr resolves."""

    def __init__(self, lib):
        for k in ("ascontiguousarray", "asarray", "zeros", "full", "zeros_like", "repeat"):
            setattr(self, k, (lambda f: lambda *a, **kw: lib.remember(f(*a, **kw)))(getattr(np, k)))

    def __getattr__(self, name):
        return getattr(np, name)


def _saopd_arena(parent, action, state, depth, reward, lower, done, count, first_child, alive, sv):
    parent[:], first_child[:], lower[4] = [-1, 0, 0, 2, 2, 2], [-1, -1, 3, -1, -1, -1], -np.inf


def _exact_plan_counts(*arrays):
    arrays[-1][:] = [3, 2, 1, 4]


class Harness(object):
    """One case's stand-in library, context and handle owners (made with object.__new__: nothing is loaded)."""

    def __init__(self, mp):
        self.lib = Lib()
        self.keep = []
        real_ptr = native._ptr
        mp.setattr(native, "_ptr", lambda a: real_ptr(self.lib.remember(a)))
        mp.setattr(native, "np", _Numpy(self.lib))
        mp.setattr(native, "_LIB", self.lib)
        mp.delenv("MP_NO_PINNED_SCRATCH", raising=False)
        mp.delenv("MP_CARTPOLE_SINCOS", raising=False)
        self.mp = mp
        self.lib.hooks.update(mp_saopd_export=_saopd_arena, mp_vi_exact_plan=_exact_plan_counts)
        self.ctx = self.lib.ctx = self.new(native.Context, _lib=self.lib, _h=C.c_void_p(CTX_H), device=0)

    def new(self, cls, **attrs):
        o = object.__new__(cls)
        o.__dict__.update(attrs)
        self.keep.append(o)
        return o

    def model(self, mode=native.MODE_DETERMINISTIC, m=1, s=S, a=A, b=0, cls=native.Model, n_models=1):
        return self.new(cls, ctx=self.ctx, _h=C.c_void_p(MODEL_H), mode=mode, M=m, S=s * n_models, A=a, B=b, _keep=None,
                        n_models=n_models, S_each=s)

    def batch_model(self):
        return self.model(n_models=4)

    def joint(self, cls=native.Model, n_models=1):
        return self.model(m=M, cls=cls, n_models=n_models)

    def policy(self, model):
        return self.new(native.Policy, ctx=self.ctx, _h=C.c_void_p(POLICY_H), model=model)

    def device_rng(self, n):
        return self.new(native.DeviceRng, ctx=self.ctx, n=n, _h=C.c_void_p(RNG_H))

    def saopd(self, n):
        return self.new(native.StateAwarePlanners, ctx=self.ctx, model=self.model(), n=n, _h=C.c_void_p(PLANNERS_H))

    def gbopd(self, n):
        return self.new(native.GraphBasedPlanners, ctx=self.ctx, model=self.model(), n=n, _h=C.c_void_p(PLANNERS_H))

    def gbop(self, n):
        return self.new(native.StochasticGraphBasedPlanners, ctx=self.ctx, model=self.model(), n=n, K=2, _h=C.c_void_p(PLANNERS_H))

    def rng(self, n):
        self.rng_state = self.lib.remember(np.arange(n * 6, dtype=np.uint64).reshape(n, 6) + 7)
        return self.rng_state

    def arr(self, values, dtype, shape=None):
        a = np.asarray(values, dtype=dtype)
        return self.lib.remember(np.ascontiguousarray(a if shape is None else np.resize(a, shape)))

    def buffers(self, *args, **kw):
        b = self.ctx.plan_buffers(*args, **kw)
        self.lib.pinned.append(b)
        return b


def _torch():
    import torch
    return torch


def _tensor(values, dtype):
    return _torch().tensor(values, dtype=getattr(_torch(), dtype))


def _tensors(n, mpl=HORIZON, **extra):
    t = _torch()
    out = dict(plans=t.zeros((n, mpl), dtype=t.int32), plan_len=t.zeros(n, dtype=t.int32), env_steps=t.zeros(n, dtype=t.int64))
    for k, (dtype, tail) in extra.items():
        out[k] = t.zeros((n,) + tail, dtype=getattr(t, dtype))
    return out


def _roots(n):
    return [i % S for i in range(n)]


PRIOR = [0.2, 0.3, 0.5]
THR = [0.5, 1.0, 1.5, 2.0, 2.5]
VIN = [4.0, 3.0, 2.0, 1.0, 0.0]
GPOW = [1.0, 0.5, 0.25, 0.125, 0.0625]
GAPE_THR = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5]                # (5 episodes + 2)

# ---- the plan methods: name -> call(h, n, **changes) ---------------------------------------------------------------


def _uct(h, n, model=None, **kw):
    kw.setdefault("rng_state", h.rng(n))
    return h.ctx.uct_plan(model or h.model(), kw.pop("root_state", _roots(n)), 5, HORIZON, 0.9, 1.0, kw.pop("prior_p", PRIOR),
                          kw.pop("rollout_p", PRIOR), **kw)


def _uct_stoch(h, n, model=None, **kw):
    kw.setdefault("rng_state", h.rng(n))
    return h.ctx.uct_plan_stochastic(model or h.model(native.MODE_STOCHASTIC), kw.pop("root_state", _roots(n)), 5, HORIZON, 0.9,
                                     1.0, kw.pop("prior_p", PRIOR), kw.pop("rollout_p", PRIOR), **kw)


def _opd(h, n, model=None, **kw):
    kw.setdefault("rng_state", h.rng(n))
    return h.ctx.opd_plan(model or h.model(), kw.pop("root_state", _roots(n)), 6, 0.9, 0.0, **kw)


def _ropd(h, n, model=None, **kw):
    kw.setdefault("rng_state", h.rng(n))
    return h.ctx.ropd_plan(model or h.joint(), kw.pop("root_state", _roots(n)), 6, 0.9, 0.0, **kw)


def _olop(h, n, model=None, method="olop_plan", **kw):
    kw.setdefault("rng_state", h.rng(n))
    return getattr(h.ctx, method)(model or h.model(), kw.pop("root_state", _roots(n)), 5, HORIZON, 0.9, kw.pop("kl", True),
                                  kw.pop("continuation", -1), kw.pop("thresholds", THR), kw.pop("value_upper_init", VIN), **kw)


def _olop_stoch(h, n, **kw):
    return _olop(h, n, model=h.model(native.MODE_STOCHASTIC), method="olop_plan_stochastic", **kw)


def _brue(h, n, model=None, **kw):
    kw.setdefault("rng_state", h.rng(n))
    return h.ctx.brue_plan(model or h.model(), kw.pop("root_state", _roots(n)), 6, HORIZON, 0.9, kw.pop("gpow", GPOW), **kw)


def _gape(h, n, model=None, method="gape_plan", stochastic=False, **kw):
    kw.setdefault("rng_state", h.rng(n))
    tables = (kw.pop("thr_by_count", GAPE_THR),) + ((kw.pop("transition_thr_by_count", GAPE_THR[::-1]),) if stochastic else ())
    return getattr(h.ctx, method)(model or h.model(), kw.pop("root_state", _roots(n)), 5, HORIZON, *((2,) if stochastic else ()),
                                  0.9, 0.5, kw.pop("uniform", True), kw.pop("n_actions_env", A), kw.pop("action_column", None),
                                  *tables, kw.pop("value_init", VIN), **kw)


def _gape_stoch(h, n, **kw):
    return _gape(h, n, model=h.model(native.MODE_SPARSE, b=2), method="gape_plan_stochastic", stochastic=True, **kw)


def _ss(h, n, model=None, **kw):
    kw.setdefault("rng_state", h.rng(n))
    return h.ctx.ss_plan(model or h.model(), kw.pop("root_state", _roots(n)), HORIZON, 2, 0.9, **kw)


def _saopd(h, n, **kw):
    kw.setdefault("rng_state", h.rng(n))
    return h.saopd(n).plan(kw.pop("root_state", _roots(n)), 6, 0.9, 0.0, **kw)


def _gbopd(h, n, **kw):
    kw.setdefault("rng_state", h.rng(n))
    return h.gbopd(n).plan(kw.pop("root_state", _roots(n)), 6, 0.9, 10.0, 0.01, HORIZON, **kw)


def _gbop(h, n, **kw):
    kw.setdefault("rng_state", h.rng(n))
    return h.gbop(n).plan(kw.pop("root_state", _roots(n)), 5, HORIZON, 0.9, 10.0, 0.01, 2, kw.pop("reward_thr", [0.0] * 5),
                          kw.pop("transition_thr", THR), **kw)


PLANS = dict(uct=_uct, uct_stoch=_uct_stoch, opd=_opd, ropd=_ropd, olop=_olop, olop_stoch=_olop_stoch, brue=_brue, ss=_ss,
             gape=_gape, gape_stoch=_gape_stoch, saopd=_saopd, gbopd=_gbopd, gbop=_gbop)
WITH_MODELS = ("uct", "opd", "olop", "brue", "ss", "gape")


def _twice(h, plan, n, **kw):
    plan(h, n, **kw)
    return plan(h, n, **kw)


def _many_shapes(h, plan):
    for mpl in range(1, 11):                                # more shapes than the context keeps scratch arrays for
        out = plan(h, 1, max_plan_len=mpl)
    return out


def _evicted_small_plan(h):
    _uct(h, 1)
    for mpl in range(1, 9):
        _opd(h, 1, max_plan_len=mpl)
    return _uct(h, 1)


def _device_plan(h, method, fixed, outputs, **kw):
    n = 2
    t = _tensors(n, **outputs)
    t.update(kw)
    rng = _tensor(np.arange(n * 6).reshape(n, 6).tolist(), "int64")
    args = [rng if a == "rng" else a for a in fixed]
    return method(*args, **t), {k: _array(v.numpy()) for k, v in sorted(t.items()) if hasattr(v, "numpy")}


UCT_OUT = dict(root_value=("float64", ()), root_child_count=("int64", (A,)), root_child_value=("float64", (A,)))
OPD_OUT = dict(root_lower=("float64", ()), root_upper=("float64", ()), status=("int32", ()))


def _uct_device(h, **kw):
    model = kw.pop("model", None) or h.model()
    return _device_plan(h, h.ctx.uct_plan_device, [model, 2, _tensor([1, 2], "int32"), 5, HORIZON, 0.9, 1.0, PRIOR, PRIOR, "rng",
                                                   HORIZON], UCT_OUT, **kw)


def _uct_stoch_device(h, **kw):
    return _device_plan(h, h.ctx.uct_plan_stochastic_device,
                        [h.model(native.MODE_STOCHASTIC), 2, _tensor([1, 2], "int32"), 5, HORIZON, 0.9, 1.0, PRIOR, PRIOR, "rng",
                         _tensor(np.arange(12).reshape(2, 6).tolist(), "int64"), HORIZON],
                        dict(root_value=("float64", ())), **kw)


def _opd_device(h, which="opd_plan_device", **kw):
    model = h.model() if which == "opd_plan_device" else h.joint()
    root = _tensor([1, 2], "int32") if which == "opd_plan_device" else _tensor([[1, 1], [2, 2]], "int32")
    return _device_plan(h, getattr(h.ctx, which), [model, 2, root, 6, 0.9, 0.0, "rng", HORIZON], OPD_OUT, **kw)


def _saopd_device(h):
    return _device_plan(h, h.saopd(2).plan_device, [_tensor([1, 2], "int32"), 6, 0.9, 0.0, "rng", HORIZON],
                        dict(updates=("int64", ()), status=("int32", ())), accuracy=0.5, prune_suboptimal_leaves=False)


def _gbopd_device(h):
    return _device_plan(h, h.gbopd(2).plan_device, [_tensor([1, 2], "int32"), 6, 0.9, 10.0, 0.01, HORIZON, "rng"],
                        dict(value_lower=("float64", ()), value_upper=("float64", ()), updates=("int64", ()),
                             status=("int32", ())))


def _gbop_device(h, rng_device_only):
    t = {k: _torch().zeros(2, dtype=getattr(_torch(), dtype)) for k, dtype in (
        ("action", "int32"), ("key", "int32"), ("plan_len", "int32"), ("value_lower", "float64"), ("value_upper", "float64"),
        ("env_steps", "int64"), ("pops", "int64"), ("status", "int32"))}
    rng = _tensor(np.arange(12).reshape(2, 6).tolist(), "int64")
    out = h.gbop(2).plan_device(_tensor([1, 2], "int32"), 5, HORIZON, 0.9, 10.0, 0.01, 2, [0.0] * 5, THR, rng,
                                rng_device_only=rng_device_only, **t)
    return out, {k: _array(v.numpy()) for k, v in sorted(t.items())}


def _gbop_graph(n, state, lower, upper, expanded, count, listed, chance_count, chance_assigned, *rest):
    """Some slots unlisted (node i lists the slots other than i % 3, node 4 none) and 0, 1 or 2 states assigned: with the two
    children mp_gbop_info reports, an odd number rotates the child order."""
    listed[:] = (np.arange(A)[None, :] != (np.arange(S) % 3)[:, None]) & (np.arange(S) != 4)[:, None]
    chance_assigned[:] = (np.arange(S)[:, None] + np.arange(A)[None, :]) % 3


def _env_step(h, stochastic, log):
    t = _torch()
    n = 2
    args = [h.model(), t.zeros(n, dtype=t.int32), t.zeros(n, dtype=t.int32), t.ones(n, dtype=t.uint8),
            t.zeros((n, HORIZON), dtype=t.int32), 9, t.ones(n, dtype=t.float64), t.zeros(n, dtype=t.float64),
            t.zeros(n, dtype=t.float64), t.zeros((n, 5), dtype=t.int32) if log else None, t.zeros(1, dtype=t.int32)]
    if stochastic:
        return h.ctx.env_step_stochastic_device(*(args + [t.zeros((n, 6), dtype=t.int64)]))
    return h.ctx.env_step_device(*args)


def _rows(h, unpack):
    t = _torch()
    arrays = [t.zeros((3, HORIZON), dtype=t.int32), t.zeros(3, dtype=t.float64)]
    if unpack:
        return h.ctx.unpack_rows(t.zeros((4, 24), dtype=t.uint8), 3, 2, arrays, stream=STREAM)
    return h.ctx.pack_rows(arrays, 3, t.zeros((2, 24), dtype=t.uint8))


def _tables(shape, offset=0):
    size = int(np.prod(shape))
    return (np.arange(size).reshape(shape) + offset) % S, (np.arange(size, dtype=np.float64).reshape(shape) + offset) / size


def _load(h, method, shape, lists=False, **kw):
    t, r = _tables(shape)
    if lists:
        t, r = t.tolist(), r.tolist()
    else:
        t, r = h.arr(t, np.int64), h.arr(r, np.float64)
    return getattr(h.ctx, method)(t, r, **kw)


def _dense(h, method, shape, device=False, terminal=None, contiguous=True):
    t = np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) / 100
    r = t[..., 0] + 1
    if device:
        t, r = _torch().tensor(t), _torch().tensor(r)
        if not contiguous:
            r = r.transpose(0, 1)
        terminal = None if terminal is None else _tensor(terminal, "uint8")
    return getattr(h.ctx, method)(t, r, terminal)


def _flags(shape):
    return (np.arange(int(np.prod(shape))).reshape(shape) % 3 == 0)


def _cartpole(h, variant):
    h.lib.returns["mp_libm_sincos_variant"] = variant
    params = dict(gravity=9.8, masscart=1.0, masspole=0.1, length=0.5, force_mag=10.0, tau=0.02, theta_threshold=0.2,
                  x_threshold=2.4, max_steps=200, euler=1)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        model = h.ctx.load_cartpole(params)
    return model, [str(x.message) for x in w]


def _failing(h, symbol, value, call):
    h.lib.returns[symbol] = value
    return call()


def _hooked(h, symbol, hook, call):
    h.lib.hooks[symbol] = hook
    return call()


def _negative_sweeps(*arrays):
    arrays[-1][:] = -1


def _closed(h, owner):
    owner.close()
    owner.close()
    return owner._h if hasattr(owner, "_h") else owner._ptr


def _missing_library(h):
    h.mp.setattr(native, "_LIB", None)
    h.mp.setenv("MI355PLAN_LIB", "/nonexistent/libmi355plan.so")
    return native.load()


def _cases():
    c = {}
    for name, plan in PLANS.items():
        for n in SIZES:
            c["{}_plan n={}".format(name, n)] = lambda h, plan=plan, n=n: plan(h, n)
            c["{}_plan n={} no_scratch".format(name, n)] = lambda h, plan=plan, n=n: (
                h.mp.setenv("MP_NO_PINNED_SCRATCH", "1"), plan(h, n))[1]
        c[name + "_plan arrays"] = lambda h, plan=plan: plan(h, 2, root_state=h.arr([3, 4], np.int32))
        c[name + "_plan bad rng dtype"] = lambda h, plan=plan: plan(h, 2, rng_state=np.zeros((2, 6), np.int64))
        c[name + "_plan bad rng size"] = lambda h, plan=plan: plan(h, 2, rng_state=np.zeros((3, 6), np.uint64))
        c[name + "_plan bad rng order"] = lambda h, plan=plan: plan(h, 2, rng_state=np.zeros((6, 2), np.uint64).T)
        c[name + "_plan bad rng list"] = lambda h, plan=plan: plan(h, 2, rng_state=[[0] * 6] * 2)
    for name in WITH_MODELS:
        for n in (2, 65):
            c["{}_plan model_index n={}".format(name, n)] = lambda h, plan=PLANS[name], n=n: plan(
                h, n, model=h.batch_model(), model_index=[i % 4 for i in range(n)])
        c[name + "_plan model_index array"] = lambda h, plan=PLANS[name]: plan(
            h, 2, model=h.batch_model(), model_index=h.arr([3, 1], np.int32))
    c["ropd_plan model_index"] = lambda h: _ropd(h, 2, model=h.joint(native.JointBatchModel, 4), model_index=[3, 1])
    c["ropd_plan roots per model"] = lambda h: _ropd(h, 2, root_state=[[1, 2], [3, 4]])
    c["ropd_plan roots per model array"] = lambda h: _ropd(h, 2, root_state=h.arr([[1, 2], [3, 4]], np.int32))
    for name in ("uct", "uct_stoch"):
        plan = PLANS[name]
        for n in (1, 65):
            c["{}_plan root_steps n={}".format(name, n)] = lambda h, plan=plan, n=n: plan(h, n, root_steps=list(range(n)))
            c["{}_plan policy n={}".format(name, n)] = lambda h, plan=plan, n=n: plan(
                h, n, model=h.model(), policy=h.policy(None), root_steps=h.arr(list(range(n)), np.int32))
        c[name + "_plan policy no steps"] = lambda h, plan=plan: plan(h, 2, policy=h.policy(None))
        c[name + "_plan prior arrays"] = lambda h, plan=plan: plan(h, 2, prior_p=h.arr(PRIOR, np.float64),
                                                                  rollout_p=h.arr(PRIOR[::-1], np.float64))
        c[name + "_plan prior shape"] = lambda h, plan=plan: plan(h, 2, prior_p=[0.5, 0.5])
        c[name + "_plan max_plan_len"] = lambda h, plan=plan: plan(h, 2, max_plan_len=2)
        c[name + "_plan device rng"] = lambda h, plan=plan: plan(h, 2, rng_state=h.device_rng(2))
        c[name + "_plan device rng short"] = lambda h, plan=plan: plan(h, 2, rng_state=h.device_rng(1))
    c["uct_plan prior shape no_scratch"] = lambda h: (h.mp.setenv("MP_NO_PINNED_SCRATCH", "1"), _uct(h, 2, rollout_p=[1.0]))[1]
    c["uct_plan twice"] = lambda h: _twice(h, _uct, 2)
    c["uct_plan twice root_steps then none"] = lambda h: (_uct(h, 2, root_steps=[1, 2]), _uct(h, 2))[1]
    c["uct_plan many shapes"] = lambda h: _many_shapes(h, _uct)
    c["uct_plan evicted small plan"] = _evicted_small_plan
    c["opd_plan twice"] = lambda h: _twice(h, _opd, 2)
    c["opd_plan many shapes"] = lambda h: _many_shapes(h, _opd)
    c["uct_plan cartpole"] = lambda h: _uct(h, 2, model=h.model(native.MODE_CARTPOLE, s=0, a=2), root_state=[[0.0, 0.1, 0.2, 0.3]] * 2,
                                            prior_p=[0.5, 0.5], rollout_p=[0.5, 0.5])
    c["uct_plan model_index policy"] = lambda h: _uct(h, 2, model=h.batch_model(), model_index=[3, 1], policy=h.policy(None))
    c["uct_plan model_index device rng"] = lambda h: _uct(h, 2, model=h.batch_model(), model_index=[3, 1],
                                                          rng_state=h.device_rng(4))
    c["uct_plan out"] = lambda h: _uct(h, 2, out=h.buffers(2, HORIZON))
    c["uct_plan out all"] = lambda h: _uct(h, 65, out=h.buffers(65, HORIZON, n_actions=A, outputs=(
        "plans", "plan_len", "root_value", "env_steps", "root_child_count", "root_child_value")))
    c["uct_plan out no plans"] = lambda h: _uct(h, 2, out=h.buffers(2, HORIZON, outputs=("root_value",)), policy=h.policy(None))
    c["uct_plan out model_index"] = lambda h: _uct(h, 2, model=h.batch_model(), model_index=[3, 1], out=h.buffers(2, HORIZON))
    c["uct_plan out wrong size"] = lambda h: _uct(h, 2, out=h.buffers(3, HORIZON))
    c["uct_plan_stochastic env rng"] = lambda h: _uct_stoch(h, 2, env_rng_state=np.arange(12, dtype=np.uint64))
    c["uct_plan_stochastic env rng list closed loop"] = lambda h: _uct_stoch(h, 2, env_rng_state=[[1] * 6] * 2, closed_loop=True)
    c["uct_plan_stochastic visits"] = lambda h: _uct_stoch(h, 2, visits=h.arr(0, np.int32, (2, S)))
    c["uct_plan_stochastic visits policy"] = lambda h: _uct_stoch(h, 2, visits=h.arr(0, np.int32, (2, S)), policy=h.policy(None),
                                                                  closed_loop=True)
    c["uct_plan_stochastic visits dtype"] = lambda h: _uct_stoch(h, 2, visits=np.zeros((2, S), np.int64))
    c["uct_plan_stochastic visits shape"] = lambda h: _uct_stoch(h, 2, visits=np.zeros((S, 2), np.int32))
    for name in ("olop", "olop_stoch"):
        plan = PLANS[name]
        c[name + "_plan no kl"] = lambda h, plan=plan: plan(h, 2, kl=False, thresholds=[], continuation=1, max_plan_len=6)
        c[name + "_plan arrays in"] = lambda h, plan=plan: plan(h, 2, thresholds=h.arr(THR, np.float64),
                                                                value_upper_init=h.arr(VIN, np.float64))
        c[name + "_plan short thresholds"] = lambda h, plan=plan: plan(h, 2, thresholds=THR[:2])
        c[name + "_plan short value_upper_init"] = lambda h, plan=plan: plan(h, 2, value_upper_init=VIN[:2])
    c["olop_plan model_index no kl"] = lambda h: _olop(h, 2, model=h.batch_model(), model_index=[3, 1], kl=False, thresholds=[])
    c["brue_plan gpow array"] = lambda h: _brue(h, 2, gpow=h.arr(GPOW, np.float64))
    c["brue_plan short gpow"] = lambda h: _brue(h, 2, gpow=GPOW[:2])
    for name in ("gape", "gape_stoch"):
        plan = PLANS[name]
        c[name + "_plan action_column"] = lambda h, plan=plan: plan(h, 2, n_actions_env=4, action_column=[2, -1, 0, 1], uniform=False)
        c[name + "_plan arrays in"] = lambda h, plan=plan: plan(h, 2, action_column=h.arr([2, 0, 1], np.int32),
                                                                thr_by_count=h.arr(GAPE_THR, np.float64),
                                                                value_init=h.arr(VIN, np.float64))
        c[name + "_plan short thr_by_count"] = lambda h, plan=plan: plan(h, 2, thr_by_count=GAPE_THR[:5])
        c[name + "_plan short value_init"] = lambda h, plan=plan: plan(h, 2, value_init=VIN[:2])
        c[name + "_plan short action_column"] = lambda h, plan=plan: plan(h, 2, n_actions_env=4, action_column=[2, 0, 1])
    c["gape_plan model_index action_column"] = lambda h: _gape(h, 2, model=h.batch_model(), model_index=[3, 1],
                                                               action_column=[2, 0, 1])
    c["gape_stoch_plan short transition_thr_by_count"] = lambda h: _gape_stoch(h, 2, transition_thr_by_count=GAPE_THR[:6])
    c["gape_stoch_plan transition array"] = lambda h: _gape_stoch(h, 2, transition_thr_by_count=h.arr(GAPE_THR, np.float64))
    c["opd_plan max_plan_len"] = lambda h: _opd(h, 2, max_plan_len=3)
    c["saopd_plan options"] = lambda h: _saopd(h, 2, accuracy=0.5, backup_aggregated_nodes=False, max_plan_len=3)
    c["saopd_plan wrong roots"] = lambda h: _saopd(h, 2, root_state=[1, 2, 3])
    c["gbopd_plan wrong roots"] = lambda h: _gbopd(h, 2, root_state=[1])
    c["gbop_plan wrong roots"] = lambda h: _gbop(h, 2, root_state=[1])
    c["gbop_plan unequal thresholds"] = lambda h: _gbop(h, 2, reward_thr=[0.0] * 4)
    c["gbop_plan threshold arrays"] = lambda h: _gbop(h, 2, reward_thr=h.arr([0.0] * 5, np.float64), transition_thr=h.arr(THR, np.float64))

    c["uct_plan_device"] = _uct_device
    c["uct_plan_device root_steps"] = lambda h: _uct_device(h, root_steps=_tensor([1, 2], "int32"))
    c["uct_plan_device policy"] = lambda h: _uct_device(h, policy=h.policy(None))
    c["uct_plan_device model_index"] = lambda h: _uct_device(h, model=h.batch_model(), model_index=_tensor([3, 1], "int32"))
    c["uct_plan_device model_index policy"] = lambda h: _uct_device(h, model_index=_tensor([3, 1], "int32"), policy=h.policy(None))
    c["uct_plan_stochastic_device"] = lambda h: _uct_stoch_device(h, closed_loop=True, root_steps=_tensor([1, 2], "int32"))
    c["uct_plan_stochastic_device policy"] = lambda h: _uct_stoch_device(h, policy=h.policy(None))
    for which in ("opd_plan_device", "ropd_plan_device"):
        c[which] = lambda h, which=which: _opd_device(h, which)
        c[which + " model_index"] = lambda h, which=which: _opd_device(h, which, model_index=_tensor([3, 1], "int32"))
    c["saopd plan_device"] = _saopd_device
    c["gbopd plan_device"] = _gbopd_device
    c["gbop plan_device"] = lambda h: _gbop_device(h, False)
    c["gbop plan_device rng only"] = lambda h: _gbop_device(h, True)

    c["uct_tree"] = lambda h: h.ctx.uct_tree(1)
    c["uct_tree cap"] = lambda h: h.ctx.uct_tree(1, cap=9)
    c["uct_stoch_tree"] = lambda h: h.ctx.uct_stoch_tree(1)
    c["opd_tree"] = lambda h: h.ctx.opd_tree(1, 9)
    c["ropd_tree"] = lambda h: h.ctx.ropd_tree(1, 9, M)
    c["olop_tree"] = lambda h: h.ctx.olop_tree(1, 9)
    c["brue_tree"] = lambda h: h.ctx.brue_tree(1, 9)
    c["ss_tree"] = lambda h: h.ctx.ss_tree(1)
    c["ss_tree cap"] = lambda h: h.ctx.ss_tree(1, cap=9)
    c["ss_tree no tree"] = lambda h: _hooked(h, "mp_ss_tree_export", lambda n, *a: setattr(n, "value", 0),
                                             lambda: _failing(h, "mp_ss_tree_export", native.MP_ERR_ARG, lambda: h.ctx.ss_tree(1)))
    for name in ("gape", "gape_stoch"):
        c[name + "_tree"] = lambda h, name=name: getattr(h.ctx, name + "_tree")(1)
        c[name + "_tree cap"] = lambda h, name=name: getattr(h.ctx, name + "_tree")(1, cap=9)
        c[name + "_tree no tree"] = lambda h, name=name: _hooked(
            h, "mp_{}_tree_export".format(name), lambda n, *a: setattr(n, "value", 0),
            lambda: _failing(h, "mp_{}_tree_export".format(name), native.MP_ERR_ARG, lambda: getattr(h.ctx, name + "_tree")(1)))
    c["saopd info"] = lambda h: h.saopd(2).info()
    c["saopd export"] = lambda h: h.saopd(2).export(1)
    c["saopd export whole arena"] = lambda h: h.saopd(2).export(0, current_tree_only=False)
    c["gbopd info"] = lambda h: h.gbopd(2).info()
    c["gbopd export"] = lambda h: h.gbopd(2).export(1)
    c["gbop info"] = lambda h: h.gbop(2).info()
    c["gbop export"] = lambda h: _hooked(h, "mp_gbop_export", _gbop_graph, lambda: h.gbop(2).export(1))
    c["gbop export every slot listed"] = lambda h: h.gbop(2).export(0)
    c["uct_step_tree"] = lambda h: h.ctx.uct_step_tree([1, 2])
    c["uct_step_tree array"] = lambda h: h.ctx.uct_step_tree(h.arr([1, 2], np.int32))
    c["uct_step_tree tensor"] = lambda h: h.ctx.uct_step_tree(_tensor([1, 2], "int32"))
    c["uct_step_tree_select"] = lambda h: h.ctx.uct_step_tree_select([0, 0, 1], h.arr([1, 2, 0], np.int32))
    c["uct_step_tree_select mismatch"] = lambda h: h.ctx.uct_step_tree_select([0, 1], [1])
    c["uct_step_tree_select tensors"] = lambda h: h.ctx.uct_step_tree_select(_tensor([0, 1], "int32"), _tensor([1, 2], "int32"))
    c["uct_step_tree_select one tensor"] = lambda h: h.ctx.uct_step_tree_select([0, 1], _tensor([1, 2], "int32"))
    c["uct_reset_tree"] = lambda h: h.ctx.uct_reset_tree()
    c["uct_path_count"] = lambda h: h.ctx.uct_path_count(1, [0, 2])
    c["uct_path_count root"] = lambda h: h.ctx.uct_path_count(1, [])

    c["load_table"] = lambda h: _load(h, "load_table", (S, A))
    c["load_table lists"] = lambda h: _load(h, "load_table", (S, A), lists=True, terminal=[0, 1] * 5, done_rule="next",
                                            max_steps=9, available=_flags((S, A)).tolist())
    c["load_table models"] = lambda h: _load(h, "load_table", (M, S, A), terminal=_flags((S,)), available=_flags((S, A)))
    c["load_table shape"] = lambda h: _load(h, "load_table", (S,))
    c["load_table mismatch"] = lambda h: h.ctx.load_table(np.zeros((S, A), np.int64), np.zeros((A, S)))
    c["load_table_batch"] = lambda h: _load(h, "load_table_batch", (4, S, A), terminal=_flags((4, S)), max_steps=9)
    c["load_table_batch lists"] = lambda h: _load(h, "load_table_batch", (4, S, A), lists=True, done_rule="next")
    c["load_table_batch shape"] = lambda h: _load(h, "load_table_batch", (S, A))
    c["load_joint"] = lambda h: _load(h, "load_joint", (M, S, A), terminals=_flags((M, S)), available=_flags((M, S, A)))
    c["load_joint lists"] = lambda h: _load(h, "load_joint", (M, S, A), lists=True, done_rule="next")
    c["load_joint shape"] = lambda h: _load(h, "load_joint", (S, A))
    c["load_joint_batch"] = lambda h: _load(h, "load_joint_batch", (4, M, S, A), terminals=_flags((4, M, S)),
                                            available=_flags((4, M, S, A)))
    c["load_joint_batch lists"] = lambda h: _load(h, "load_joint_batch", (4, M, S, A), lists=True, done_rule="next")
    c["load_joint_batch shape"] = lambda h: _load(h, "load_joint_batch", (M, S, A))
    for method in ("load_dense", "load_dense_rows"):
        c[method] = lambda h, method=method: _dense(h, method, (S, A, S), terminal=[1, 0] * 5)
        c[method + " models"] = lambda h, method=method: _dense(h, method, (M, S, A, S))
        c[method + " device"] = lambda h, method=method: _dense(h, method, (S, A, S), device=True, terminal=[1, 0] * 5)
        c[method + " device strided"] = lambda h, method=method: _dense(h, method, (A, A, A), device=True, contiguous=False)
    c["load_dense shape"] = lambda h: _dense(h, "load_dense", (S, A, S + 1))
    c["load_dense ndim"] = lambda h: _dense(h, "load_dense", (S, S))
    c["load_dense_rows block"] = lambda h: _dense(h, "load_dense_rows", (M, 4, A, S), terminal=_flags((4,)))
    c["load_sparse"] = lambda h: h.ctx.load_sparse(_tables((S, A, 2))[1], _tables((S, A, 2))[0], _tables((S, A))[1], _flags((S,)))
    c["load_sparse lists"] = lambda h: h.ctx.load_sparse(_tables((S, A, 2))[1].tolist(), _tables((S, A, 2))[0].tolist(),
                                                         _tables((S, A))[1].tolist())
    c["load_sparse shape"] = lambda h: h.ctx.load_sparse(_tables((S, A, 2))[1], _tables((S, A))[0], _tables((S, A))[1])
    c["load_cartpole"] = lambda h: _cartpole(h, 1)
    c["load_cartpole own sincos"] = lambda h: _cartpole(h, 0)
    c["load_policy"] = lambda h: h.ctx.load_policy(h.model(), _tables((S, A))[1], _tables((S, A), 1)[1])
    c["load_policy shared lists"] = lambda h: (lambda p: h.ctx.load_policy(h.model(), p, p, listed=_flags((S, A)).tolist(),
                                                                         rollout_slots=(_tables((S, A))[0] % A).tolist()))(
        _tables((S, A))[1].tolist())
    c["load_policy arrays"] = lambda h: h.ctx.load_policy(h.model(), h.arr(_tables((S, A))[1], np.float64),
                                                          h.arr(_tables((S, A), 1)[1], np.float64), listed=_flags((S, A)),
                                                          rollout_slots=h.arr(_tables((S, A))[0] % A, np.uint8))
    c["load_policy batch rows"] = lambda h: h.ctx.load_policy(h.batch_model(), _tables((S, A))[1], _tables((S, A), 1)[1])
    c["load_policy batch global"] = lambda h: h.ctx.load_policy(h.batch_model(), _tables((4 * S, A))[1], _tables((4 * S, A), 1)[1])
    c["load_policy shape"] = lambda h: h.ctx.load_policy(h.model(), _tables((S, A))[1], _tables((A, S))[1])
    c["model set_available"] = lambda h: (lambda m: (m.set_available(_flags((S, A)).tolist()), m.available))(h.model())[1]
    c["model update_tables"] = lambda h: h.model().update_tables(0, *(_tables((1, S, A)) + (_flags((1, S)),)))
    c["model update_tables batch lists"] = lambda h: h.batch_model().update_tables(1, *[x.tolist() for x in _tables((2, S, A))])
    c["model update_rows"] = lambda h: h.batch_model().update_rows([3, 12], *(_tables((2, A)) + ([1, 0],)))
    c["model update_rows arrays"] = lambda h: h.batch_model().update_rows(h.arr([3, 12], np.int32), h.arr(_tables((2, A))[0], np.int64),
                                                                          h.arr(_tables((2, A))[1], np.float64))
    c["model update_rows repeated"] = lambda h: h.batch_model().update_rows([3, 3], *_tables((2, A)))
    c["model set_episode_rules"] = lambda h: h.model().set_episode_rules("next", 9)
    c["joint batch set_available"] = lambda h: (lambda m: (m.set_available(_flags((4, M, S, A))), m.available))(
        h.joint(native.JointBatchModel, 4))[1]
    c["joint batch update_tables"] = lambda h: h.joint(native.JointBatchModel, 4).update_tables(
        1, *(_tables((2, M, S, A)) + (_flags((2, M, S)),)))
    c["joint batch update_tables lists"] = lambda h: h.joint(native.JointBatchModel, 4).update_tables(
        1, *[x.tolist() for x in _tables((2, M, S, A))])

    c["vi_solve"] = lambda h: h.ctx.vi_solve(h.model(), 0.9, 20, robust=True)
    c["vi_solve failed"] = lambda h: _hooked(h, "mp_vi_solve", _negative_sweeps, lambda: h.ctx.vi_solve(h.model(), 0.9, 20))
    c["vi_solve_v"] = lambda h: h.ctx.vi_solve_v(h.model(), 0.9, 20)
    c["vi_solve_v robust"] = lambda h: h.ctx.vi_solve_v(h.model(), 0.9, 20, robust=True)
    c["vi_solve_device"] = lambda h: h.ctx.vi_solve_device(h.model(), 0.9, 20, _torch().zeros((S, A), dtype=_torch().float64),
                                                           _tensor([0], "int32"))
    c["vi_solve_batch"] = lambda h: h.ctx.vi_solve_batch(h.batch_model(), 0.9, 20)
    c["vi_solve_batch_device"] = lambda h: h.ctx.vi_solve_batch_device(
        h.batch_model(), 0.9, 20, _torch().zeros((4 * S, A), dtype=_torch().float64), _tensor([0] * 4, "int32"))
    c["vi_sweeps"] = lambda h: h.ctx.vi_sweeps(h.model(), 0.9, 3, robust=True)
    c["vi_dense_mode"] = lambda h: h.ctx.vi_dense_mode("exact")
    c["vi_backup"] = lambda h: h.ctx.vi_backup(h.model(), 0.9, list(range(S)))
    c["vi_backup q_out"] = lambda h: h.ctx.vi_backup(h.model(), 0.9, h.arr(range(S), np.float64), q_out=h.arr(0, np.float64, (S, A)),
                                                     robust=True)
    c["vi_backup device"] = lambda h: _array(h.ctx.vi_backup(h.model(), 0.9, _torch().zeros(S, dtype=_torch().float64),
                                                             q_out=_torch().zeros((S, A), dtype=_torch().float64)).numpy())
    c["check_device_sweeps"] = lambda h: native.check_device_sweeps(_tensor([4], "int32"))
    c["check_device_sweeps failed"] = lambda h: native.check_device_sweeps(_tensor([-1], "int32"))

    c["context create"] = lambda h: (lambda ctx: (ctx._h.value, ctx.device, h.keep.append(ctx)))(native.Context(1, STREAM))[:2]
    c["context create default stream"] = lambda h: (lambda ctx: (ctx._h.value, h.keep.append(ctx)))(native.Context())[:1]
    c["context close"] = lambda h: (_uct(h, 1), _closed(h, h.ctx))[1]
    c["synchronize"] = lambda h: h.ctx.synchronize()
    c["synchronize failed"] = lambda h: _failing(h, "mp_ctx_synchronize", native.MP_ERR_ARG, h.ctx.synchronize)
    c["device_faults"] = lambda h: h.ctx.device_faults()
    c["set_stream"] = lambda h: (h.ctx.set_stream(STREAM), h.ctx.set_stream(None))
    c["stream_ptr"] = lambda h: h.ctx.stream_ptr()
    c["device_info"] = lambda h: h.ctx.device_info()
    c["last_kernel_ms"] = lambda h: h.ctx.last_kernel_ms()
    c["last_kernel_variant"] = lambda h: h.ctx.last_kernel_variant()
    c["vi_graph_captures"] = lambda h: h.ctx.vi_graph_captures()
    c["comm"] = lambda h: (lambda uid: (h.ctx.comm_init(1, 2, uid), h.ctx.comm_destroy(), uid))(native.Context.comm_unique_id())[2]
    c["gather_results"] = lambda h: h.ctx.gather_results(_torch().zeros((2, 24), dtype=_torch().uint8),
                                                         _torch().zeros((4, 24), dtype=_torch().uint8), stream=STREAM)
    c["selftest_sincos"] = lambda h: h.ctx.selftest_sincos([0.1, 0.2], 1)
    c["selftest_olop_bound log"] = lambda h: h.ctx.selftest_olop_bound("log", [1.0, 2.0])
    c["selftest_olop_bound kl"] = lambda h: h.ctx.selftest_olop_bound("bernoulli_kl", [0.1, 0.2], [0.3, 0.4])
    c["selftest_olop_bound kl lengths"] = lambda h: h.ctx.selftest_olop_bound("bernoulli_kl", [0.1, 0.2], [0.3])
    c["selftest_olop_bound upper"] = lambda h: h.ctx.selftest_olop_bound("kl_upper_bound", [0.1, 0.2], [0.3, 0.4], [1, 2])
    c["selftest_olop_bound upper lengths"] = lambda h: h.ctx.selftest_olop_bound("kl_upper_bound", [0.1, 0.2], [0.3, 0.4], [1])
    c["selftest_lds_atomic_order"] = lambda h: h.ctx.selftest_lds_atomic_order(128)
    c["pinned"] = lambda h: (lambda p: (sorted(p), p.nbytes, _closed(h, p), len(p)))(
        h.ctx.pinned(dict(a=((3,), np.int32), b=((2, 2), np.float64))))
    c["plan_buffers"] = lambda h: h.buffers(3, HORIZON, n_actions=A, outputs=("plans", "root_child_count", "root_lower", "status"))
    c["device_rng int"] = lambda h: (lambda r: (r.n, r._h.value, h.keep.append(r)))(h.ctx.device_rng(3))[:2]
    c["device_rng states"] = lambda h: (lambda r: (r.n, h.keep.append(r)))(h.ctx.device_rng(np.arange(12).tolist()))[:1]
    c["device rng get set"] = lambda h: (lambda r: (r.set(np.arange(6, dtype=np.uint64), first=1), r.get(), r.get(1, 1), r.ptr(1)))(
        h.device_rng(3))
    c["device rng seed_sequence"] = lambda h: (lambda r: (r.seed_sequence([1, 2 ** 40], first_key=3), r.seed_sequence((), 0, 1, 1)))(
        h.device_rng(3))
    c["device rng no pointer"] = lambda h: _failing(h, "mp_rng_device_ptr", None, lambda: h.device_rng(3).ptr(9))
    c["env_step_device"] = lambda h: _env_step(h, False, True)
    c["env_step_device no log"] = lambda h: _env_step(h, False, False)
    c["env_step_stochastic_device"] = lambda h: _env_step(h, True, True)
    c["env_step_stochastic_device no log"] = lambda h: _env_step(h, True, False)
    c["greedy_actions_device"] = lambda h: h.ctx.greedy_actions_device(
        _torch().zeros((S, A), dtype=_torch().float64), _tensor([1, 2], "int32"), _torch().zeros((2, HORIZON), dtype=_torch().int32))
    c["pack_rows"] = lambda h: _rows(h, False)
    c["unpack_rows"] = lambda h: _rows(h, True)
    for name, owner in (("model", lambda h: h.model()), ("policy", lambda h: h.policy(None)), ("device rng", lambda h: h.device_rng(2)),
                        ("saopd", lambda h: h.saopd(2)), ("gbopd", lambda h: h.gbopd(2)), ("gbop", lambda h: h.gbop(2))):
        c[name + " close"] = lambda h, owner=owner: _closed(h, owner(h))
        c[name + " close after context"] = lambda h, owner=owner: (lambda o: (setattr(h.ctx, "_h", None), _closed(h, o)))(owner(h))[1]
    c["saopd create"] = lambda h: (lambda p: (p.n, p._h.value, h.keep.append(p)))(native.StateAwarePlanners(h.ctx, h.model(), 2))[:2]
    c["gbopd create"] = lambda h: (lambda p: (p.n, p._h.value, h.keep.append(p)))(native.GraphBasedPlanners(h.ctx, h.model(), 2))[:2]
    c["gbopd create queue"] = lambda h: (lambda p: (p.n, h.keep.append(p)))(native.GraphBasedPlanners(h.ctx, h.model(), 2, 32))[:1]
    c["gbop create"] = lambda h: (lambda p: (p.n, p.K, p._h.value, h.keep.append(p)))(
        native.StochasticGraphBasedPlanners(h.ctx, h.model(native.MODE_SPARSE, b=2), 2, 3))[:3]
    c["gbop create queue"] = lambda h: (lambda p: (p.n, p.K, h.keep.append(p)))(
        native.StochasticGraphBasedPlanners(h.ctx, h.model(), 2, 3, 32))[:2]

    c["seed_sequence_states"] = lambda h: native.seed_sequence_states([1, 2 ** 40], 3, 2)
    c["seed_sequence_states no entropy"] = lambda h: native.seed_sequence_states((), 3, 2)
    c["entropy_words"] = lambda h: native.entropy_words(0)
    c["entropy_words negative"] = lambda h: native.entropy_words([1, -1])
    c["libm_sincos"] = lambda h: (native.libm_sincos_variant(), native.libm_sincos([0.1, 0.2], 2))
    c["olop_allocation"] = lambda h: native.olop_allocation(100, 0.9)
    c["olop_allocation failed"] = lambda h: _failing(h, "mp_olop_allocation", -4, lambda: native.olop_allocation(1, 0.9))
    c["uct_choose_form"] = lambda h: native.uct_choose_form(list(range(len(native.UCT_CALL_FIELDS))))
    c["saopd_choose_form"] = lambda h: native.saopd_choose_form(list(range(len(native.SAOPD_CALL_FIELDS))))
    c["form names"] =lambda h: [f() for f in (native.kernel_form_names, native.each_form_names, native.olop_stoch_form_names,
                                               native.ss_form_names, native.ss_each_form_names, native.vi_form_names)]
    c["each_form_info"] = lambda h: native.each_form_info("ss", S, A, HORIZON, 2)
    c["ss_geometry"] = lambda h: native.ss_geometry(A, HORIZON, 2, 1)
    c["vi_geometry deterministic"] = lambda h: native.vi_geometry("deterministic", S, A, M)
    c["vi_geometry stochastic"] = lambda h: _hooked(h, "mp_vi_geometry", lambda out: out.__setitem__(slice(10, 12), [1, 2]),
                                                    lambda: native.vi_geometry("stochastic", S, A, Sc=16))
    c["vi_batch_geometry"] = lambda h: _hooked(h, "mp_vi_batch_geometry", lambda out, name: out.__setitem__(0, 1),
                                               lambda: native.vi_batch_geometry(5, S, A, 200))
    c["vi_exact_plan"] = lambda h: native.vi_exact_plan(20)
    c["rng_state_from_generator"] = lambda h: native.rng_state_from_generator(np.random.Generator(np.random.PCG64(5)))
    c["rng_state_from_generator other"] = lambda h: native.rng_state_from_generator(np.random.Generator(np.random.MT19937(5)))
    c["generator_set_state"] = lambda h: (lambda g: (native.generator_set_state(g, np.arange(6, dtype=np.uint64) + 1),
                                                     native.rng_state_from_generator(g)))(np.random.Generator(np.random.PCG64(5)))[1]
    c["_ptr of a list"] = lambda h: native._ptr([1, 2])
    c["load without a library"] = _missing_library
    return c


CASES = _cases()


def _describe(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, bytes):
        return v.decode()
    if isinstance(v, np.ndarray):
        return _array(v) + ["own" if v.flags.owndata else "view"]
    if isinstance(v, np.generic):
        return [type(v).__name__, v.item()]
    if isinstance(v, native.PinnedArrays):
        return ["PinnedArrays", v.nbytes, {k: _describe(a) for k, a in v.items()}]
    if isinstance(v, dict):
        return {k: _describe(a) for k, a in v.items()}
    if isinstance(v, (list, tuple)):
        return [_describe(a) for a in v]
    if isinstance(v, (native.Model, native.Policy, native.DeviceRng)):
        d = {k: _describe(a) for k, a in sorted(vars(v).items()) if k not in ("ctx", "model")}
        return [type(v).__name__, d, {k: type(a).__name__ for k, a in vars(v).items() if k in ("ctx", "model")}]
    if isinstance(v, C.c_void_p):
        return ["c_void_p", v.value]
    if hasattr(v, "data_ptr"):
        return ["tensor", str(v.dtype), list(v.shape)]
    raise TypeError("cannot describe {!r}".format(type(v)))


def run_case(name, mp):
    h = Harness(mp)
    rec = {}
    try:
        rec["result"] = _describe(CASES[name](h))
    except Exception as e:     # noqa: BLE001 - type and message are the record
        rec["error"] = [type(e).__name__, str(e), getattr(e, "code", None)]
    rec["calls"] = list(h.lib.calls)
    if hasattr(h, "rng_state"):
        rec["rng_after"] = _array(h.rng_state)
    mp.undo()                   # (handles that die from here on call into a stand-in nobody reads)
    return json.loads(json.dumps(rec))


@functools.lru_cache(maxsize=None)
def _expected():
    with open(RECORD) as f:
        return json.load(f)


def test_record_holds_exactly_the_cases():
    assert sorted(_expected()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_binding_call(name, monkeypatch):
    expected = _expected()[name]
    got = run_case(name, monkeypatch)
    assert json.dumps(got, sort_keys=True) == json.dumps(expected, sort_keys=True)


def record_all():
    out = {}
    for name in sorted(CASES):
        mp = pytest.MonkeyPatch()
        try:
            out[name] = run_case(name, mp)
        finally:
            mp.undo()
    return out


def unreached_lines():
    """Lines of native.py's functions that no case executes (sys.settrace)."""
    path, hit, lines = native.__file__, set(), set()

    def trace(frame, event, arg):
        if frame.f_code.co_filename != path:
            return None
        hit.add(frame.f_lineno)
        return trace

    sys.settrace(trace)
    try:
        record_all()
    finally:
        sys.settrace(None)

    def walk(code):
        if code.co_flags & 1:                               # (a function's body: class bodies ran at import)
            lines.update(ln for _, _, ln in code.co_lines() if ln)
        for c in code.co_consts:
            if hasattr(c, "co_lines"):
                walk(c)

    with open(path) as f:
        source = f.read()
    for c in compile(source, path, "exec").co_consts:
        if hasattr(c, "co_lines"):
            walk(c)
    text = source.split("\n")
    return [(ln, text[ln - 1]) for ln in sorted(lines - hit) if not text[ln - 1].lstrip().startswith("def ")]


if __name__ == "__main__":
    if sys.argv[1:] == ["--unreached"]:
        for ln, text in unreached_lines():
            print("{:5d} {}".format(ln, text[:120]))
        sys.exit(0)
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_binding_calls_host.py --write | --unreached   (the native.py first on PYTHONPATH: "
                 "--write records its calls, --unreached lists its lines that no case runs)")
    with open(RECORD, "w") as f:
        f.write("{\n" + ",\n".join("{}:{}".format(json.dumps(k), json.dumps(v, sort_keys=True, separators=(",", ":")))
                                  for k, v in sorted(record_all().items())) + "\n}\n")
    print("wrote {} cases to {}".format(len(CASES), RECORD))
