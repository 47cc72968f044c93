"""Call traces of tclip_amd.engine on the CPU: `_capi.lib` is replaced by a fake library that records every call, and each
argument is rendered without addresses - struct fields, scalar type and value, array values, `null`, `ws`, the workspace size,
the stream, and every pointer (the members of a TaskSource too) resolved through data_ptr to the name of the input it was passed
or the position of the output the function returned.  A pointer that resolves to nothing fails the recording: the inputs are
contiguous and of their final dtype, so the engine copies none of them.

tests/golden/engine_call_traces.json was recorded with this file from engine.py as it stood before its few-shot families
were folded into one runner per method; tests/test_engine_call_traces.py replays the cases and compares for equality.  The
fixture is never regenerated.  To repeat the recording against another checkout of the package:

    PYTHONPATH=<checkout>/transductive-clip_amd python tests/helpers/engine_trace.py <new file>
"""
import contextlib
import ctypes
import inspect
import itertools
import json

import torch

T, Q, S, K, D, ROWS = 2, 5, 4, 3, 8, 20
WS_BYTES = 12544


class Recorder:
    """The fake library: every tclip_* attribute is a function that records its name and arguments, returns WS_BYTES from a
    workspace query and 0 from an entry"""

    def __init__(self):
        self.calls = []
        self.stream = ctypes.c_void_p(0)

    def __getattr__(self, name):
        if not name.startswith("tclip_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        self.calls.append((name, [self._freeze(a) for a in args]))
        if name == "tclip_last_error":
            return b""
        return WS_BYTES if name.endswith("_workspace_bytes") else 0

    def _freeze(self, a):
        """what the argument holds at the time of the call; addresses are resolved once the outputs are known"""
        if a is None:
            return ("text", "null")
        if a is self.stream:
            return ("text", "stream")
        if type(a).__name__ == "CArgObject":                    # ctypes.byref(struct)
            s = a._obj
            fields = [(f, getattr(s, f)) for f, _ in s._fields_]
            if type(s).__name__ == "TaskSource":
                return ("struct", "TaskSource", [(f, ("ptr", v) if v is not None else ("text", "null")) for f, v in fields])
            return ("struct", type(s).__name__, [(f, ("text", repr(list(v) if isinstance(v, ctypes.Array) else v))) for f, v in fields])
        if isinstance(a, ctypes.c_void_p):
            return ("ptr", a.value) if a.value else ("text", "null")
        if isinstance(a, ctypes.Array):
            return ("text", f"{a._type_.__name__}[{len(a)}]({', '.join(repr(v) for v in a)})")
        if isinstance(a, ctypes._SimpleCData):
            return ("text", f"{type(a).__name__}({a.value!r})")
        if isinstance(a, int) and not isinstance(a, bool):
            return ("text", f"ws_bytes({a})" if a == WS_BYTES else f"int({a})")
        raise AssertionError(f"an argument of type {type(a).__name__} reached the library")

    def entries(self):
        return [name for name, _ in self.calls if not name.endswith("_workspace_bytes")]


def install(monkeypatch, engine):
    """the patches that let engine.py run on CPU tensors -> the Recorder in the library's place"""
    rec = Recorder()
    monkeypatch.setattr(engine._capi, "lib", lambda: rec)
    monkeypatch.setattr(engine, "_require_cuda", lambda t, name: None)
    monkeypatch.setattr(engine, "_stream", lambda: rec.stream)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: None)
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, stream: None)
    return rec


def _resolve(calls, names):
    out = []
    for name, args in calls:
        def text(a, last=False):
            if a[0] == "text":
                return a[1]
            if a[0] == "struct":
                return f"{a[1]}({', '.join(f'{f}={text(v)}' for f, v in a[2])})"
            if a[1] in names:
                return names[a[1]]
            if last and a[1] % 256 == 0:                       # the aligned view of the workspace: no input, no output
                return "ws"
            raise AssertionError(f"{name}: a pointer that is neither an input nor an output")
        tail = len(args) >= 3 and args[-1] == ("text", "stream") and args[-2] == ("text", f"ws_bytes({WS_BYTES})")
        out.append([name] + [text(a, last=tail and i == len(args) - 3) for i, a in enumerate(args)])
    return out


def _outputs(result):
    if isinstance(result, tuple):
        return [(f"out[{i}]", t) for i, t in enumerate(result)]
    return [(f"out.{f}", getattr(result, f)) for f in type(result).__slots__]


def run(rec, engine, fn, inp, pos, kw):
    """one call -> {"calls": [[name, arg, ...], ...], "returns": {...}} or {"refused": "Type: message"}"""
    del rec.calls[:]
    try:
        result = getattr(engine, fn)(*[inp[n] if n is not None else None for n in pos], **kw)
    except Exception as e:      # noqa: BLE001  - every refusal is recorded by type and message
        assert not rec.entries(), f"{fn}: {rec.entries()} ran before the refusal"
        return {"refused": f"{type(e).__name__}: {e}", "calls_before": [name for name, _ in rec.calls]}
    names = {t.data_ptr(): f"in.{n}" for n, t in inp.items()}
    outs = _outputs(result)
    for n, t in outs:
        assert t.data_ptr() not in names, f"{fn}: {n} shares its address with {names[t.data_ptr()]}"
        names[t.data_ptr()] = n
    return {"calls": _resolve(rec.calls, names),
            "returns": {n: f"{str(t.dtype).replace('torch.', '')} {tuple(t.shape)}" for n, t in outs}}


# ---- the inputs: contiguous, in their final dtype ------------------------------------------------------------------------------

def inputs(width, tables):
    g = torch.Generator().manual_seed(width)
    y_s = torch.tensor([[0, 1, 2, 0], [2, 1, 0, 1]])
    if not tables:
        return {"x_q": torch.rand(T, Q, width, generator=g), "x_s": torch.rand(T, S, width, generator=g), "y_s": y_s}
    inp = {"table_q": torch.rand(ROWS, width, generator=g), "q_idx": torch.arange(T * Q).reshape(T, Q) * 3 % ROWS,
           "table_s": torch.rand(ROWS, width, generator=g), "s_idx": torch.arange(T * S).reshape(T, S) * 7 % ROWS, "y_s": y_s}
    if width == K:
        inp["cols"] = torch.tensor([[2, 0, 1], [1, 2, 0]], dtype=torch.int32)
    return inp


def _set(name, make):
    def fault(inp, kw):
        inp[name] = make(inp)
    return fault


def _kw(**changes):
    return lambda inp, kw: kw.update(changes)


def _width(inp):
    return inp["table_q" if "table_q" in inp else "x_q"].shape[-1]


def _bad_label(inp):
    y_s = inp["y_s"].clone()
    if y_s.numel():
        y_s[0, 0] = K
    return y_s


def _no_support(inp, kw):
    inp["y_s"] = torch.zeros(T, 0, dtype=torch.int64)
    if "s_idx" in inp:
        inp["s_idx"] = torch.zeros(T, 0, dtype=torch.int64)
    else:
        inp["x_s"] = torch.zeros(T, 0, _width(inp))


def _cols_range(inp):
    cols = inp["cols"].clone()
    cols[1, 1] = cols.shape[1]
    return cols


def _idx_range(name):
    def make(inp):
        idx = inp[name].clone()
        idx.view(-1)[-1] = ROWS
        return idx
    return make


FAULTS = {
    "x_s_tasks": _set("x_s", lambda inp: torch.zeros(T + 1, S, _width(inp))),
    "x_s_width": _set("x_s", lambda inp: torch.zeros(T, S, _width(inp) + 1)),
    "y_s_shape": _set("y_s", lambda inp: torch.zeros(T, S + 1, dtype=torch.int64)),
    "label": _set("y_s", _bad_label),
    "no_support": _no_support,
    "n_class_low": _kw(n_class=1),
    "n_class_high": _kw(n_class=1025),
    "norm_type": _kw(norm_type="XX"),
    "norm_cl2n": _kw(norm_type="CL2N"),
    "entropy": _kw(entropies=("Shannon", "Renyi", "Alpha")),
    "n_batches": _kw(n_batches=3),
    "q_idx_dims": _set("q_idx", lambda inp: inp["q_idx"].reshape(-1).clone()),
    "table_s_width": _set("table_s", lambda inp: torch.zeros(ROWS, _width(inp) + 1)),
    "q_idx_range": _set("q_idx", _idx_range("q_idx")),
    "s_idx_range": _set("s_idx", _idx_range("s_idx")),
    "s_idx_tasks": _set("s_idx", lambda inp: torch.zeros(T + 1, S, dtype=torch.int64)),
    "cols_shape": _set("cols", lambda inp: torch.zeros(T, _width(inp) + 1, dtype=torch.int32)),
    "cols_range": _set("cols", _cols_range),
    "cols_visual": _set("cols", lambda inp: torch.zeros(T, _width(inp), dtype=torch.int32)),
    "values_empty": _kw(values=[]),
    "values_nan": _kw(values=[1.5, float("nan")]),
    "values_scalar": _kw(values=3.0),
}

DENSE, TAB = ("x_q", "x_s", "y_s"), ("table_q", "q_idx", "table_s", "s_idx", "y_s")
TABC = TAB + ("cols",)
F_DENSE = ("x_s_tasks", "x_s_width", "y_s_shape")
F_DENSE_VISUAL = F_DENSE + ("n_class_low", "n_class_high", "label")
F_TAB = ("q_idx_dims", "table_s_width", "q_idx_range", "s_idx_range", "no_support", "s_idx_tasks", "y_s_shape", "label")
F_COLS = ("cols_shape", "cols_range")
F_N_CLASS = ("n_class_low", "n_class_high")
F_VALUES = ("values_empty", "values_nan", "values_scalar")
LW = (1.0, 0.5, 0.25)


def _family(stem, kw, swept, faults=(), n_batches=False):
    """the five entry kinds of a method with a sweep, on both feature kinds -> [(case, fn, width, tables, pos, kw, faults)]"""
    nb = ("n_batches",) if n_batches else ()
    one = dict(kw, **{swept: 0.5})
    many = dict(kw, values=[1.5, 2.5])
    vis = {"n_class": K}
    return [
        (f"run_{stem}", f"run_{stem}", K, False, DENSE, one, faults + F_DENSE + nb),
        (f"run_{stem}_visual", f"run_{stem}_visual", D, False, DENSE, dict(one, **vis),
         faults + F_DENSE_VISUAL + nb + (("no_support",) if stem == "alpha_tim" else ())),
        (f"run_{stem}_tasks", f"run_{stem}_tasks", K, True, TAB, one, ()),
        (f"run_{stem}_tasks+cols", f"run_{stem}_tasks", K, True, TABC, one, faults + F_TAB + F_COLS + nb),
        (f"run_{stem}_visual_tasks", f"run_{stem}_visual_tasks", D, True, TAB, dict(one, **vis), faults + F_N_CLASS + F_TAB + nb),
        (f"sweep_{stem}_tasks", f"sweep_{stem}_tasks", K, True, TAB, many, ()),
        (f"sweep_{stem}_tasks+cols", f"sweep_{stem}_tasks", K, True, TABC, many, F_VALUES + faults + F_TAB + F_COLS + nb),
        (f"sweep_{stem}_tasks+n_class", f"sweep_{stem}_tasks", D, True, TAB, dict(many, **vis),
         F_VALUES + faults + F_N_CLASS + ("cols_visual",) + F_TAB + nb),
    ]


def cases():
    tim = dict(iters=3, temp=15.0, lr=1e-3, loss_weights=LW, n_batches=2)
    gd = dict(tim, n_class=K)
    em = dict(n_batches=2, iters=3, iter_mm=7, lambd=9.0, hard=True)
    return (
        _family("paddle", dict(iters=3), "lambd")
        + _family("bdcspn", dict(norm_type="CL2N"), "temp", ("norm_type",))
        + _family("laplacian_shot", dict(iters=3, knn=3, norm_type="UN"), "lmd", ("norm_type", "norm_cl2n"))
        + _family("alpha_tim", tim, "alpha_value", ("entropy",), n_batches=True)
        + [("run_tim_gd", "run_tim_gd", K, False, DENSE, gd, ("no_support",) + F_DENSE_VISUAL + ("n_batches",)),
           ("run_tim_gd+visual", "run_tim_gd", D, False, DENSE, gd, ()),
           ("run_tim_gd_tasks", "run_tim_gd_tasks", K, True, TAB, gd, ()),
           ("run_tim_gd_tasks+cols", "run_tim_gd_tasks", K, True, TABC, gd, F_N_CLASS + F_TAB + F_COLS + ("n_batches",)),
           ("run_tim_gd_tasks+visual", "run_tim_gd_tasks", D, True, TAB, gd, F_N_CLASS + ("cols_visual",) + F_TAB + ("n_batches",)),
           ("run_em_dirichlet", "run_em_dirichlet", K, False, ("x_q",), em, ("n_batches",)),
           ("run_em_dirichlet+support", "run_em_dirichlet", K, False, DENSE, em, ("n_batches",) + F_DENSE),
           ("run_em_dirichlet_tasks", "run_em_dirichlet_tasks", K, True, ("table_q", "q_idx"), em, ("q_idx_range", "n_batches")),
           ("run_em_dirichlet_tasks+cols", "run_em_dirichlet_tasks", K, True, ("table_q", "q_idx", None, None, None, "cols"), em,
            ("q_idx_range", "n_batches") + F_COLS),
           ("run_em_dirichlet_tasks+support", "run_em_dirichlet_tasks", K, True, TAB, em, ()),
           ("run_em_dirichlet_tasks+support+cols", "run_em_dirichlet_tasks", K, True, TABC, em,
            ("q_idx_range", "n_batches", "table_s_width", "s_idx_range", "s_idx_tasks", "y_s_shape") + F_COLS)])


def public_surface(engine):
    """{name: signature and doc of every public function and class of engine, the value of every public constant}"""
    out = {}
    for name, obj in sorted(vars(engine).items()):
        if name.startswith("_") or inspect.ismodule(obj):
            continue
        if inspect.isfunction(obj):
            out[name] = {"signature": str(inspect.signature(obj)), "doc": inspect.getdoc(obj)}
        elif inspect.isclass(obj):
            out[name] = {"signature": str(inspect.signature(obj)), "doc": inspect.cleandoc(obj.__doc__) if obj.__doc__ else None}
        else:
            out[name] = {"value": repr(obj)}
    return out


def record(monkeypatch, engine):
    """every case, each of its refusals alone and every pair of them (which of two refusals comes first), the public surface"""
    rec = install(monkeypatch, engine)
    traces, refusals = {}, {}
    for case, fn, width, tables, pos, kw, faults in cases():
        traces[case] = run(rec, engine, fn, inputs(width, tables), pos, dict(kw))
        assert "calls" in traces[case], f"{case}: {traces[case]}"
        for combo in [(f,) for f in faults] + list(itertools.combinations(faults, 2)):
            inp, bad_kw = inputs(width, tables), dict(kw)
            bad_pos = pos + (("cols",) if "cols_visual" in combo else ())
            for f in combo:
                FAULTS[f](inp, bad_kw)
            got = run(rec, engine, fn, inp, bad_pos, bad_kw)
            refusals.setdefault(case, {})["+".join(combo)] = (got["refused"] if "refused" in got and not got["calls_before"]
                                                              else "not refused in Python" if "calls" in got else got)
    return {"public": public_surface(engine), "traces": traces, "refusals": refusals}


def dumps(recording):
    return json.dumps(recording, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    import os
    import sys

    import pytest
    from tclip_amd import engine
    if len(sys.argv) != 2 or os.path.exists(sys.argv[1]):
        sys.exit("usage: engine_trace.py NEW_FILE  (an existing file is never overwritten)")
    with pytest.MonkeyPatch.context() as mp:
        text = dumps(record(mp, engine))
    with open(sys.argv[1], "w") as f:
        f.write(text)
