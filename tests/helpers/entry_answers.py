"""What the 29 run entries and 26 workspace queries of the nine k-means / few-shot methods answer before any HIP call: the
sizes the queries return over a grid of problems, and the code and message of every single argument fault of a run entry and of
every pair of them.  tests/golden/method_entry_answers.json holds these answers as the library gave them before the entries were
folded onto one check path per method; tests/test_entry_answers.py replays them.

Every run call here carries at least one fault, so no call reaches a launch: the device pointers are the integer 4096 and are
never dereferenced.  The host structs (problem, task source, TIM parameters, loss weights, sweep values) are real."""
import ctypes
import itertools
import json

from tclip_amd import _capi

PTR = 4096
BIG = 1 << 40                     # workspace size passed when the query itself rejects the problem
DIM = 9
# T = 6, K = 5, Q = 7, S = 11, D = 9: no workspace region of any layout is a multiple of 256 bytes
PROBLEM = dict(n_batches=2, tasks_per_batch=3, n_query=7, n_class=5, n_support=11, iters=3, iter_mm=1, lambd=150, hard=0)

ZS, FS = "zero-shot", "few-shot"
# name -> (method, kind, arguments after the problem, workspace query, flags).  Argument words: dim method knn norm nv are int32,
# f a float, d a double, prm / lw / src / values the host structs, ws wsb stream the tail; any other word is a device pointer.
# Flags: iters = iters 0 is a fault, int32 = the entry has an int32 limit beyond tclip_problem's, cols = cols given is a fault,
# opt:<pointer> = this pointer may be null in this variant.
_KM = "x_q u0 f u v w preds criterions ws wsb stream"
RUNS = {
    "tclip_soft_kmeans_run": ("SOFT_KMEANS", ZS, "x_q f u w preds ws wsb stream", "tclip_soft_kmeans_workspace_bytes", ""),
    "tclip_em_gaussian_run": ("EM_GAUSSIAN", ZS, "x_q f u v w preds ws wsb stream", "tclip_soft_kmeans_workspace_bytes", ""),
    "tclip_hard_kmeans_run": ("HARD_KMEANS", ZS, "x_q u w preds criterions ws wsb stream", "tclip_hard_kmeans_workspace_bytes", ""),
    "tclip_em_gaussian_cov_run": ("EM_GAUSSIAN_COV", ZS, "x_q u v w s preds ws wsb stream", "tclip_soft_kmeans_workspace_bytes", ""),
    "tclip_kl_kmeans_run": ("KL_KMEANS", ZS, "x_q u w preds criterions ws wsb stream", "tclip_hard_kmeans_workspace_bytes", ""),
    "tclip_kmeans_visual_run|soft": ("SOFT_KMEANS", ZS, "dim method=0 " + _KM, "tclip_visual_workspace_bytes", "opt:v opt:criterions"),
    "tclip_kmeans_visual_run|hard": ("HARD_KMEANS", ZS, "dim method=1 " + _KM, "tclip_visual_workspace_bytes", "opt:v"),
    "tclip_kmeans_visual_run|emg": ("EM_GAUSSIAN", ZS, "dim method=2 " + _KM, "tclip_visual_workspace_bytes", "opt:criterions"),
    "tclip_em_gaussian_cov_visual_run": ("EM_GAUSSIAN_COV", ZS, "dim x_q u0 u v w s preds ws wsb stream",
                                         "tclip_em_gaussian_cov_visual_workspace_bytes", ""),
}
_SWEEP = {"|prob": ("dim=0", ""), "|visual": ("dim", " cols")}


def _few_shot(stem, method, scalar, outs, extra_flags="", params="", swept=True, sweep_scalar=None):
    """the five call forms of a few-shot method; `scalar`: the words of its tunable scalars, in a sweep `sweep_scalar`"""
    vis = "int32 " if method in ("PADDLE", "BDCSPN", "ALPHA_TIM") else ""
    tail = f"{outs} ws wsb stream"
    pre = params + " " if params else ""
    RUNS[f"tclip_{stem}_run"] = (method, FS, f"{pre}x_q x_s y_s {scalar} {tail}", f"tclip_{stem}_workspace_bytes", extra_flags)
    RUNS[f"tclip_{stem}_visual_run"] = (method, FS, f"dim {pre}x_q x_s y_s {scalar} {tail}", f"tclip_{stem}_visual_workspace_bytes",
                                       vis + extra_flags)
    RUNS[f"tclip_{stem}_run_tasks"] = (method, FS, f"{pre}src y_s {scalar} {tail}", f"tclip_{stem}_tasks_workspace_bytes", extra_flags)
    RUNS[f"tclip_{stem}_visual_run_tasks"] = (method, FS, f"dim {pre}src y_s {scalar} {tail}",
                                             f"tclip_{stem}_visual_tasks_workspace_bytes", vis + "cols " + extra_flags)
    if swept:
        for variant, (dim, cols) in _SWEEP.items():
            RUNS[f"tclip_{stem}_sweep_tasks{variant}"] = (method, FS, f"{dim} {pre}src y_s {sweep_scalar} {tail}",
                                                         f"tclip_{stem}_sweep_tasks_workspace_bytes", "int32" + cols + " " + extra_flags)


_few_shot("paddle", "PADDLE", "f", "u v w preds", sweep_scalar="values nv")
_few_shot("bdcspn", "BDCSPN", "f norm", "prototypes u preds", sweep_scalar="values nv norm")
_few_shot("alpha_tim", "ALPHA_TIM", "", "weights logits_q preds criterions", extra_flags="iters", params="prm", sweep_scalar="values nv")
_few_shot("laplacian_shot", "LAPLACIAN_SHOT", "knn d norm", "unary neighbours preds_iter energies", extra_flags="iters",
          sweep_scalar="knn values nv norm")
RUNS["tclip_tim_gd_run"] = ("TIM_GD", FS, "dim d f lw x_q x_s y_s weights logits_q preds criterions ws wsb stream",
                            "tclip_tim_gd_workspace_bytes", "iters int32")
RUNS["tclip_tim_gd_run_tasks"] = ("TIM_GD", FS, "dim d f lw src y_s weights logits_q preds criterions ws wsb stream",
                                  "tclip_tim_gd_tasks_workspace_bytes", "iters int32 cols")
METHODS = sorted({r[0] for r in RUNS.values()})
QUERIES = sorted({r[3] for r in RUNS.values()})
_INTS = ("dim", "method", "knn", "norm", "nv")


def _state(kind):
    return dict(p=dict(PROBLEM, n_support=PROBLEM["n_support"] if kind == FS else 0), dim=DIM, method=0, knn=3, norm=1, nv=3,
                values=[0.5, 2.0, 3.0], entropies=[0, 1, 0], alpha=2.0, null=set(), cols=False, ws_short=0, ws_off=0)


def _set(**kw):
    def apply(s):
        for k, v in kw.items():
            if k in s["p"]:
                s["p"][k] = v
            else:
                s[k] = v
    return apply


def _null(word):
    return lambda s: s["null"].add(word)


def _entropy(i):
    def apply(s):
        s["entropies"][i] = 7
    return apply


def _alpha_one(sweep):
    def apply(s):
        if sweep:
            s["values"][1] = 1.0
        else:
            s["alpha"] = 1.0
    return apply


def _value(v):
    def apply(s):
        s["values"][1] = v
    return apply


def faults(name):
    """[(fault name, mutation of the call state)] of one run entry, in a fixed order"""
    _, kind, spec, _, flags = RUNS[name]
    words = [w.split("=")[0] for w in spec.split()]
    flags = flags.split()
    sweep = "values" in words
    out = []
    for w in words:
        if w in _INTS or w in ("f", "d", "wsb", "stream") or "opt:" + w in flags:
            continue
        out.append(("null:" + w, _null(w)))
        if w == "src":
            out += [("null:src." + m, _null("src." + m)) for m in ("table_q", "q_idx", "table_s", "s_idx")]
    if "cols" in flags:
        out.append(("cols", _set(cols=True)))
    if "prm" in words:
        out += [(f"entropy{i}", _entropy(i)) for i in range(3)] + [("alpha1", _alpha_one(sweep))]
    if sweep:
        T = PROBLEM["n_batches"] * PROBLEM["tasks_per_batch"]
        out += [("value:inf", _value(float("inf"))), ("value:nan", _value(float("nan"))), ("nv0", _set(nv=0)),
                ("nvcap", _set(nv=65535 // T + 1))]
    if "dim" in words and "dim=0" not in spec.split():
        out += [("dim-1", _set(dim=-1)), ("dim1025", _set(dim=1025))] + ([] if sweep else [("dim0", _set(dim=0))])
    if "dim=0" in spec.split():
        out += [("dim-1", _set(dim=-1)), ("dim1025", _set(dim=1025))]
    if "method" in words:
        out.append(("method99", _set(method=99)))
    if "knn" in words:
        out += [("knn1", _set(knn=1)), ("knnQ+1", lambda s: s.update(knn=s["p"]["n_query"] + 1)), ("q1025", _set(n_query=1025)),
                ("lds", _set(n_query=1000, knn=20))]
    if "norm" in words:
        out.append(("norm7", _set(norm=7)))
    if "iters" in flags:
        out.append(("iters0", _set(iters=0)))
    out.append(("support+", _set(n_support=5)) if kind == ZS else ("support0", _set(n_support=0)))
    if "int32" in flags:
        out.append(("int32", _set(n_batches=65535, tasks_per_batch=1, n_support=16000, n_query=40000)))
    out += [("ws-1", _set(ws_short=1)), ("ws+128", _set(ws_off=128))]
    return out


def _message(lib):
    return lib.tclip_last_error().decode()


def _query(lib, query, s):
    p = _capi.Problem(**s["p"])
    n = len(_capi._SIGNATURES[query][1])
    return getattr(lib, query)(ctypes.byref(p), *([s["dim"], s["nv"]][:n - 1]))


def call(lib, name, mutations):
    """(code, message) of run entry `name` with `mutations` applied, in order, to its valid base call"""
    _, kind, spec, query, _ = RUNS[name]
    s = _state(kind)
    for w in spec.split():
        if "=" in w:
            s[w.split("=")[0]] = int(w.split("=")[1])
    for m in mutations:
        m(s)
    p = _capi.Problem(**s["p"])
    src = _capi.TaskSource(*[None if "src." + m in s["null"] else PTR for m in ("table_q", "q_idx", "table_s", "s_idx")],
                           PTR if s["cols"] else None)
    prm = _capi.TimParams(1e-3, 15.0, s["alpha"], (ctypes.c_float * 3)(1.0, 1.0, 1.0), (ctypes.c_int32 * 3)(*s["entropies"]))
    lw = (ctypes.c_float * 3)(1.0, 0.3, 1.0)
    values = (ctypes.c_double * len(s["values"]))(*s["values"])
    size = _query(lib, query, s) or BIG
    args = []
    for w in (w.split("=")[0] for w in spec.split()):
        if w in s["null"]:
            args.append(None)
        elif w in _INTS:
            args.append(s[w])
        elif w == "f":
            args.append(ctypes.c_float(1.5))
        elif w == "d":
            args.append(ctypes.c_double(0.75))
        elif w in ("prm", "src"):
            args.append(ctypes.byref(prm if w == "prm" else src))
        elif w in ("lw", "values"):
            args.append(lw if w == "lw" else values)
        elif w == "ws":
            args.append(ctypes.c_void_p(PTR + s["ws_off"]))
        elif w == "wsb":
            args.append(size - s["ws_short"])
        elif w == "stream":
            args.append(None)
        else:
            args.append(ctypes.c_void_p(PTR))
    rc = getattr(lib, name.split("|")[0])(ctypes.byref(p), *args)
    return rc, _message(lib)


_GRID = dict(n_batches=[1, 5], tasks_per_batch=[1, 4, 32768], n_query=[1, 76, 1025], n_support=[0, 1, 16, 16001],
             n_class=[1, 2, 37, 1024, 1025], dim=[0, 1, 16, 1024, 1025, -1], nv=[0, 1, 2, 10922, 10923, 65535])


def query_grid(query):
    """the problems one query is asked about: the base, every single move and every pair of moves of two different sizes"""
    n = len(_capi._SIGNATURES[query][1])
    kind = ZS if any(r[3] == query and r[1] == ZS for r in RUNS.values()) else FS
    names = [k for k in _GRID if k not in ("dim", "nv")] + ["dim", "nv"][:n - 1]
    base = _state(kind)
    moves = [(k, v) for k in names for v in _GRID[k] if v != (base["p"][k] if k in base["p"] else base[k])]
    return [()] + [(m,) for m in moves] + [(a, b) for a, b in itertools.combinations(moves, 2) if a[0] != b[0]]


def ask(lib, query, moves):
    """the size `query` returns for the base problem after `moves`, or the message of its refusal"""
    kind = ZS if any(r[3] == query and r[1] == ZS for r in RUNS.values()) else FS
    s = _state(kind)
    for k, v in moves:
        _set(**{k: v})(s)
    return _query(lib, query, s) or _message(lib)


def record(lib):
    """the fixture's content from `lib`: messages once, in a table; answers as sizes or negated 1-based message numbers"""
    messages = []

    def msg(text):
        if text not in messages:
            messages.append(text)
        return messages.index(text)

    out = {"messages": messages, "queries": {}, "runs": {}}
    for q in QUERIES:
        out["queries"][q] = [a if isinstance(a, int) else -1 - msg(a) for a in (ask(lib, q, m) for m in query_grid(q))]
    for name in RUNS:
        fl = faults(name)
        single = [call(lib, name, [m]) for _, m in fl]
        pairs = [call(lib, name, [a[1], b[1]]) for a, b in itertools.combinations(fl, 2)]
        for (rc, text), what in zip(single + pairs, [f[0] for f in fl] + [a[0] + "+" + b[0] for a, b in itertools.combinations(fl, 2)]):
            assert rc in (1, 2), f"{name} {what}: every recorded call must be refused before a HIP call, got {rc} ({text})"
        out["runs"][name] = {"faults": [f[0] for f in fl], "single": [[rc, msg(t)] for rc, t in single],
                             "pairs": [[rc, msg(t)] for rc, t in pairs]}
    return out


def dumps(rec):
    return json.dumps(rec, separators=(",", ":")).replace('},"', '},\n"').replace('],"tclip', '],\n"tclip') + "\n"


if __name__ == "__main__":          # python tests/helpers/entry_answers.py OUT.json, with TCLIP_LIB naming the library to record
    import sys
    with open(sys.argv[1], "w") as f:
        f.write(dumps(record(_capi.lib())))
