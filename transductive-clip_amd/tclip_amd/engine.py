"""Host-side driver of the HIP engine: torch tensors in, torch tensors out.

PyTorch is plumbing here (device memory through its caching allocator, the current HIP stream);
every number is produced by libtclip.so.  One call handles n_batches independent reference
batches (the MM stop test couples the tasks of one batch, so the batch is the
unit of parity and of multi-GPU sharding).

The few-shot methods follow the host loops of the library: one runner per method (`_paddle`, `_bdcspn`, `_laplacian_shot`,
`_alpha_tim`, `_tim_gd`, `_em_dirichlet`) holds the method's Problem, outputs and C argument tuple once, and is fed by a `_Rows`
that says where the task rows come from - dense tensors or feature tables.  The public run_* / sweep_* functions check their
arguments, build the `_Rows` and make one runner call."""
import collections
import ctypes

import torch

from . import _capi


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU: the EM-Dirichlet engine has no CPU path")


class EMDirichletResult:
    __slots__ = ("u", "v", "alpha", "preds", "criterions", "mm_iters")

    def __init__(self, **kw):
        for k, val in kw.items():
            setattr(self, k, val)


class _Call:
    """One engine call: workspace from PyTorch's caching allocator (256-byte aligned view), output tensors on
    the inputs' device, the entry point launched on the current stream, the workspace kept alive until that
    stream has consumed it.  `args(ws_ptr, ws_bytes, stream)` builds the C argument tuple."""

    def __init__(self, dev, problem, ws_query, *ws_args):
        self.dev, self.p, self.lib = dev, problem, _capi.lib()
        self.ws_bytes = getattr(self.lib, ws_query)(ctypes.byref(problem), *ws_args)
        if self.ws_bytes == 0:
            raise RuntimeError(f"{ws_query} rejected the problem: " + self.lib.tclip_last_error().decode())

    def empty(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.dev)

    def launch(self, entry, args):
        with torch.cuda.device(self.dev):
            ws = torch.empty(self.ws_bytes + 256, dtype=torch.uint8, device=self.dev)
            off = (-ws.data_ptr()) % 256
            rc = getattr(self.lib, entry)(ctypes.byref(self.p), *args(ctypes.c_void_p(ws.data_ptr() + off), self.ws_bytes, _stream()))
            _capi.check(rc, entry)
            ws.record_stream(torch.cuda.current_stream())


def _query(x_q, name="x_q"):
    _require_cuda(x_q, name)
    return x_q.contiguous().float()


def _support(x_q, x_s, y_s):
    _require_cuda(x_s, "x_s")
    _require_cuda(y_s, "y_s")
    x_s = x_s.contiguous().float()
    y_s = y_s.reshape(x_s.shape[0], -1).contiguous().long()
    T, _, K = x_q.shape
    if x_s.shape[0] != T or x_s.shape[2] != K or y_s.shape != x_s.shape[:2]:
        raise ValueError("x_s must be (T,S,K) and y_s (T,S) with the T and K of x_q")
    return x_s, y_s


def _check_n_class(n_class):
    n_class = int(n_class)
    if not 2 <= n_class <= 1024:
        raise ValueError("n_class must be in 2..1024")
    return n_class


def _support_visual(x_q, x_s, y_s, n_class):
    """_support for D-wide rows: the width of x_s is checked against D, the labels against n_class (on the device: one
    reduction, its result read back, so that no kernel ever sees a label outside 0..n_class-1)."""
    x_s, y_s = _support(x_q, x_s, y_s.to(x_q.device))
    n_class = _check_n_class(n_class)
    if y_s.numel() and not bool(((y_s >= 0) & (y_s < n_class)).all()):
        raise ValueError(f"y_s holds a label outside 0..{n_class - 1}")
    return x_s, y_s, n_class


# ---- where the task rows of a few-shot call come from ------------------------------------------------------------------------
# dev, the task shape (T, Q, S, D: S = 0 without a support set, D the row width), y_s (T,S) int64 on dev or None, `args`: the
# leading C arguments that name the rows, `run` / `ws_query`: the suffixes of the entry and of its workspace query, `keep`: every
# prepared tensor and the struct `args` points into - whoever holds the _Rows keeps them alive until the launch has happened.
_Rows = collections.namedtuple("_Rows", "dev T Q S D y_s args run ws_query keep")


def _dense_rows(x_q, x_s=None, y_s=None):
    """The rows of dense tensors: x_q (T,Q,D) as `_query`, x_s (T,S,D) and y_s as `_support` / `_support_visual` return them."""
    T, Q, D = x_q.shape
    return _Rows(x_q.device, T, Q, x_s.shape[1] if x_s is not None else 0, D, y_s, (_ptr(x_q), _ptr(x_s)), "_run",
                 "_workspace_bytes", (x_q, x_s))


def _table_rows(table_q, q_idx, table_s, s_idx, y_s, cols):
    """The rows read in place from the feature tables (struct tclip_task_source): checked tensors on one device, table_s None
    without a support set (S = 0), cols None without a column permutation."""
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    src = _capi.TaskSource(ptr(table_q), ptr(q_idx), ptr(table_s), ptr(s_idx), ptr(cols))
    T, Q = q_idx.shape
    return _Rows(table_q.device, T, Q, s_idx.shape[1] if table_s is not None else 0, table_q.shape[1], y_s, (ctypes.byref(src),),
                 "_run_tasks", "_tasks_workspace_bytes", (src, table_q, q_idx, table_s, s_idx, cols))


def _rows_call(stem, rows, problem, visual, values=None, infix="_visual"):
    """The call of a few-shot method on `rows` -> (call, entry, dim, P).  A single-value call: the entry and the workspace query
    are stem [+ infix on visual features] + the suffixes of `rows`, dim = (D,) on visual features and () on probability ones,
    P = ().  With `values` (the array of `_sweep_values`): stem + _sweep_tasks, dim = (D or 0,) always, P = (n_values,), the
    leading dimension of the outputs that depend on the value."""
    if values is None:
        dim = (ctypes.c_int32(rows.D),) if visual else ()
        stem += infix if visual else ""
        return _Call(rows.dev, problem, stem + rows.ws_query, *dim), stem + rows.run, dim, ()
    dim = (ctypes.c_int32(rows.D if visual else 0),)
    call = _Call(rows.dev, problem, stem + "_sweep_tasks_workspace_bytes", *dim, ctypes.c_int32(len(values)))
    return call, stem + "_sweep_tasks", dim, (len(values),)


def _swept(values, ctype=None, scalar=None):
    """what stands in a method's C tuple where its tunable parameter goes: (values, n_values) of a sweep, or the scalar as a
    `ctype` (nothing for ALPHA_TIM, whose alpha_value travels in its struct)"""
    if values is not None:
        return values, ctypes.c_int32(len(values))
    return (ctype(float(scalar)),) if ctype is not None else ()


def _em_dirichlet(rows, K, n_batches, iters, iter_mm, lambd, hard):
    """EM-Dirichlet on `rows`, zero-shot (S = 0) or few-shot: tclip_em_dirichlet_run / tclip_em_dirichlet_run_tasks"""
    T, Q, dev = rows.T, rows.Q, rows.dev
    c = _Call(dev, _capi.Problem(n_batches, T // n_batches, Q, K, rows.S, iters, iter_mm, int(lambd), int(bool(hard))),
              "tclip_workspace_bytes")
    u, v, alpha, preds = c.empty(T, Q, K), c.empty(T, K), c.empty(T, K, K), c.empty(T, Q, dtype=torch.int32)
    crit = torch.zeros(n_batches, max(iters, 1), device=dev)[:, :iters].contiguous()
    mm = torch.zeros(n_batches, max(iters, 1), dtype=torch.int32, device=dev)[:, :iters].contiguous()
    c.launch("tclip_em_dirichlet" + rows.run, lambda ws, n, st: (*rows.args, _ptr(rows.y_s), _ptr(u), _ptr(v), _ptr(alpha),
                                                                 _ptr(preds), _ptr(crit), _ptr(mm), ws, n, st))
    return EMDirichletResult(u=u, v=v, alpha=alpha, preds=preds, criterions=crit, mm_iters=mm)


def run_em_dirichlet(x_q, x_s=None, y_s=None, *, n_batches=1, iters, iter_mm=1000, lambd, hard=False):
    """x_q (T,Q,K) f32 cuda with T = n_batches * tasks_per_batch; x_s (T,S,K), y_s (T,S) for few-shot.

    Returns EMDirichletResult of cuda tensors; nothing is synchronised."""
    x_q = _query(x_q)
    T, _, K = x_q.shape
    if T % n_batches:
        raise ValueError("number of tasks must be a multiple of n_batches")
    if x_s is not None:
        x_s, y_s = _support(x_q, x_s, y_s.to(x_q.device))
    return _em_dirichlet(_dense_rows(x_q, x_s, y_s), K, n_batches, iters, iter_mm, lambd, hard)


def _check_on_device(idx, n_rows, cols, n_class, name):
    """tclip_check_task_indices on device-resident tensors: IndexError where torch's own `table[idx]` would raise one
    (TCLIP_ERR_INDEX only; a bad argument is a RuntimeError like every other failed call).  Negative values are rejected,
    not wrapped as torch wraps them - on the host path (`_index_tensor`) too.  The call waits for the stream: one host
    synchronisation per checked tensor."""
    with torch.cuda.device(idx.device if idx is not None else cols.device):
        rc = _capi.lib().tclip_check_task_indices(_ptr(idx) if idx is not None else None, idx.numel() if idx is not None else 0, max(1, int(n_rows)),
                                                  _ptr(cols) if cols is not None else None, cols.numel() if cols is not None else 0, int(n_class), _stream())
    if rc == 4:                             # TCLIP_ERR_INDEX
        raise IndexError(f"{name}: {_capi.lib().tclip_last_error().decode()}")
    _capi.check(rc, "tclip_check_task_indices")


def _index_tensor(idx, n_rows, dev, name):
    """int64 (T,R) index tensor on the device, every value checked against the table's row count as torch's own
    `table[idx]` checks it (IndexError; negative values are rejected, not wrapped): on the host when that is where the tensor
    is (the samplers produce CPU tensors), by one pass on the device otherwise (tclip_check_task_indices, which synchronises
    the stream: a caller that keeps its index tensors on the device pays one host sync per call)"""
    idx = idx.long()
    if not idx.is_cuda:
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n_rows):
            raise IndexError(f"{name}: index out of range for a table of {n_rows} rows")
        return idx.to(dev).contiguous()
    idx = idx.to(dev).contiguous()
    if idx.numel():
        _check_on_device(idx, n_rows, None, 1, name)
    return idx


def run_em_dirichlet_tasks(table_q, q_idx, table_s=None, s_idx=None, y_s=None, cols=None, *, n_batches=1, iters, iter_mm=1000,
                           lambd, hard=False):
    """The loop of run_em_dirichlet fed from the task-batch loop's feature tables (tclip_em_dirichlet_run_tasks):
    table_q (rows,K) f32 cuda, q_idx (T,Q) rows of it; few-shot: table_s, s_idx (T,S), y_s (T,S) the re-indexed support
    labels; cols (T,K) the per-task column permutation of Tasks_Generator_few_shot.get_task or None.  No (T,S,K) /
    (T,Q,K) tensor is built; the results are those of run_em_dirichlet on the materialised tensors, bit for bit."""
    rows, K = _em_dirichlet_table_rows(table_q, q_idx, table_s, s_idx, y_s, cols, n_batches)
    return _em_dirichlet(rows, K, n_batches, iters, iter_mm, lambd, hard)


def _em_dirichlet_table_rows(table_q, q_idx, table_s, s_idx, y_s, cols, n_batches):
    """The argument checks of run_em_dirichlet_tasks (tclip_amd.until_stable shares them) -> (the `_Rows` of the tables, K)"""
    # the checks of `_task_tables` in this entry's own order and words (it has no label check, and its support set may be absent)
    _require_cuda(table_q, "table_q")
    table_q = table_q.contiguous().float()
    dev, K = table_q.device, table_q.shape[1]
    q_idx = _index_tensor(q_idx, table_q.shape[0], dev, "q_idx")
    T, _ = q_idx.shape
    if T % n_batches:
        raise ValueError("number of tasks must be a multiple of n_batches")
    if table_s is not None:
        _require_cuda(table_s, "table_s")
        table_s = table_s.contiguous().float()
        s_idx = _index_tensor(s_idx, table_s.shape[0], dev, "s_idx")
        S = s_idx.shape[1]
        y_s = y_s.reshape(T, -1).long().to(dev).contiguous()
        if table_s.shape[1] != K or s_idx.shape[0] != T or tuple(y_s.shape) != (T, S):
            raise ValueError("table_s must be (rows,K), s_idx and y_s (T,S) with the T of q_idx")
    if cols is not None:
        cols = cols.to(torch.int32)
        if tuple(cols.shape) != (T, K) or (not cols.is_cuda and (int(cols.min()) < 0 or int(cols.max()) >= K)):
            raise IndexError("cols must be (T,K) with values in [0, K)")
        on_device = cols.is_cuda
        cols = cols.to(dev).contiguous()
        if on_device:
            _check_on_device(None, 1, cols, K, "cols")
    return _table_rows(table_q, q_idx, table_s, s_idx, y_s, cols), K


def _cols_tensor(cols, T, W, dev):
    """int32 (T,W) column permutations on the device, every value checked against the row width: on the host when that is
    where the tensor is, by tclip_check_task_indices otherwise (IndexError, as `_index_tensor`)"""
    cols = cols.to(torch.int32)
    if tuple(cols.shape) != (T, W) or (not cols.is_cuda and cols.numel() and (int(cols.min()) < 0 or int(cols.max()) >= W)):
        raise IndexError(f"cols must be (T,{W}) with values in [0, {W})")
    on_device = cols.is_cuda
    cols = cols.to(dev).contiguous()
    if on_device and cols.numel():
        _check_on_device(None, 1, cols, W, "cols")
    return cols


def gather_task_rows(table, idx, cols=None):
    """The fused task builder (tclip_gather_task_rows): table (n,W) f32 cuda, idx (T,R) int64 rows of it, cols (T,W) the per-task
    column permutation of Tasks_Generator_few_shot.get_task or None -> (T,R,W) f32 cuda with out[t,r,d] =
    table[idx[t,r], cols[t,d]]: `table[idx][..., cols]` in one pass, a bit-exact copy.  An index or column outside its range
    raises IndexError before anything is launched.  Not synchronised (device-resident idx / cols: one host sync each for the
    range check)."""
    _require_cuda(table, "table")
    if table.dim() != 2 or idx.dim() != 2:
        raise ValueError("table must be (n,W) and idx (T,R)")
    table = table.contiguous().float()
    dev, W = table.device, table.shape[1]
    idx = _index_tensor(idx, table.shape[0], dev, "idx")
    T, R = idx.shape
    if cols is not None:
        cols = _cols_tensor(cols, T, W, dev)
    out = torch.empty(T, R, W, device=dev)
    if out.numel() == 0:
        return out
    with torch.cuda.device(dev):
        rc = _capi.lib().tclip_gather_task_rows(_ptr(table), table.shape[0], W, _ptr(idx), R, _ptr(cols), T * R, _ptr(out), _stream())
    _capi.check(rc, "tclip_gather_task_rows")
    return out


def _kmeans_call(x_q, K, ws_query, *ws_args, iters, lambd=0, n_batches=1):
    """What the zero-shot k-means calls share on either feature kind: the problem, the workspace query and the outputs every
    method has.  x_q (T,Q,D), D = K for probability features -> (call, u (T,Q,K), w (T,K,D), preds (T,Q) i32)."""
    T, Q, D = x_q.shape
    if T % n_batches:
        raise ValueError("the number of tasks must be a multiple of n_batches")
    c = _Call(x_q.device, _capi.Problem(n_batches, T // n_batches, Q, K, 0, iters, 1, int(lambd), 0), ws_query, *ws_args)
    return c, c.empty(T, Q, K), c.empty(T, K, D), c.empty(T, Q, dtype=torch.int32)


def run_soft_kmeans(x_q, *, iters, temperature):
    """SOFT_KMEANS: x_q (T,Q,K) f32 cuda -> (u (T,Q,K), w (T,K,K), preds (T,Q) i32), cuda, not synchronised."""
    x_q = _query(x_q)
    c, u, w, preds = _kmeans_call(x_q, x_q.shape[2], "tclip_soft_kmeans_workspace_bytes", iters=iters)
    c.launch("tclip_soft_kmeans_run", lambda ws, n, st: (_ptr(x_q), ctypes.c_float(float(temperature)), _ptr(u), _ptr(w),
                                                         _ptr(preds), ws, n, st))
    return u, w, preds


def run_em_gaussian(x_q, *, iters, temperature, lambd):
    """EM_GAUSSIAN: x_q (T,Q,K) f32 cuda -> (u (T,Q,K), v (T,K), w (T,K,K), preds (T,Q) i32), cuda,
    not synchronised."""
    x_q = _query(x_q)
    T, _, K = x_q.shape
    c, u, w, preds = _kmeans_call(x_q, K, "tclip_soft_kmeans_workspace_bytes", iters=iters, lambd=lambd)
    v = c.empty(T, K)
    c.launch("tclip_em_gaussian_run", lambda ws, n, st: (_ptr(x_q), ctypes.c_float(float(temperature)), _ptr(u), _ptr(v),
                                                         _ptr(w), _ptr(preds), ws, n, st))
    return u, v, w, preds


def run_em_gaussian_cov(x_q, *, iters, lambd):
    """EM_GAUSSIAN_COV: x_q (T,Q,K) f32 cuda -> (u (T,Q,K), v (T,K), w (T,K,K), s (T,K,K), preds (T,Q) i32),
    cuda, not synchronised."""
    x_q = _query(x_q)
    T, _, K = x_q.shape
    c, u, w, preds = _kmeans_call(x_q, K, "tclip_soft_kmeans_workspace_bytes", iters=iters, lambd=lambd)
    v, s = c.empty(T, K), c.empty(T, K, K)
    c.launch("tclip_em_gaussian_cov_run", lambda ws, n, st: (_ptr(x_q), _ptr(u), _ptr(v), _ptr(w), _ptr(s), _ptr(preds), ws, n, st))
    return u, v, w, s, preds


def _run_hard(entry, x_q, iters, n_batches):
    """HARD_KMEANS and KL_KMEANS: the same arguments, workspace and outputs"""
    x_q = _query(x_q)
    c, u, w, preds = _kmeans_call(x_q, x_q.shape[2], "tclip_hard_kmeans_workspace_bytes", iters=iters, n_batches=n_batches)
    crit = c.empty(n_batches, iters)
    c.launch(entry, lambda ws, n, st: (_ptr(x_q), _ptr(u), _ptr(w), _ptr(preds), _ptr(crit), ws, n, st))
    return u, w, preds, crit


def run_kl_kmeans(x_q, *, iters, n_batches=1):
    """KL_KMEANS: same outputs as run_hard_kmeans."""
    return _run_hard("tclip_kl_kmeans_run", x_q, iters, n_batches)


def run_hard_kmeans(x_q, *, iters, n_batches=1):
    """HARD_KMEANS: x_q (T,Q,K) f32 cuda -> (u one-hot (T,Q,K), w (T,K,K), preds (T,Q) i32,
    criterions (n_batches, iters)), cuda, not synchronised."""
    return _run_hard("tclip_hard_kmeans_run", x_q, iters, n_batches)


def _task_tables(table_q, q_idx, table_s, s_idx, y_s, cols, K, method):
    """What the few-shot entries fed from the feature tables share: the tables as contiguous f32 (rows,D) tensors of one width on
    one device, the index tensors and cols range-checked (IndexError) and on that device, the labels checked against K.
    -> their `_Rows`"""
    _require_cuda(table_q, "table_q")
    _require_cuda(table_s, "table_s")
    if table_q.dim() != 2 or table_s.dim() != 2 or q_idx.dim() != 2 or s_idx.dim() != 2:
        raise ValueError("table_q and table_s must be (rows,D), q_idx (T,Q) and s_idx (T,S)")
    table_q, table_s = table_q.contiguous().float(), table_s.contiguous().float()
    dev, D = table_q.device, table_q.shape[1]
    if table_s.shape[1] != D or table_s.device != dev:
        raise ValueError("table_q and table_s must be (rows,D) tensors of one width on one device")
    q_idx = _index_tensor(q_idx, table_q.shape[0], dev, "q_idx")
    s_idx = _index_tensor(s_idx, table_s.shape[0], dev, "s_idx")
    T = q_idx.shape[0]
    S = s_idx.shape[1]
    if S < 1:
        raise ValueError(f"{method} is a few-shot method: s_idx must be (T,S) with n_support = S positive")
    y_s = y_s.reshape(y_s.shape[0], -1).long().to(dev).contiguous()
    if s_idx.shape[0] != T or tuple(y_s.shape) != (T, S):
        raise ValueError("s_idx and y_s must be (T,S) with the T of q_idx")
    if y_s.numel() and not bool(((y_s >= 0) & (y_s < K)).all()):
        raise ValueError(f"y_s holds a label outside 0..{K - 1}")
    if cols is not None:
        cols = _cols_tensor(cols, T, D, dev)
    return _table_rows(table_q, q_idx, table_s, s_idx, y_s, cols)


# ---- value sweeps: the four tunable few-shot methods for a list of values on the same tasks (tclip_*_sweep_tasks) ----------
def _sweep_values(values, name):
    """the list of values as a C double array; ValueError for an empty list or a value that is not a finite number - before
    anything touches the device"""
    import math
    try:
        vals = [float(v) for v in values]
    except TypeError:
        raise ValueError(f"{name} must be a non-empty list of finite numbers")
    if not vals or not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{name} must be a non-empty list of finite numbers")
    return (ctypes.c_double * len(vals))(*vals)


def _sweep_n_class(table_q, n_class, cols, method):
    """(K, visual): n_class=None is the probability form (K = the tables' width), a number the visual one, which has no cols"""
    if n_class is None:
        return (table_q.shape[1] if table_q.dim() == 2 else 0), False
    n_class = _check_n_class(n_class)
    if cols is not None:
        raise ValueError(f"{method} on visual features permutes no columns: cols must be None")
    return n_class, True


# ---- PADDLE --------------------------------------------------------------------------------------------------------------------
def _paddle(rows, K, visual, iters, lambd, values=None):
    """PADDLE on rows of D elements: tclip_paddle[_visual]_run[_tasks] with lambd, tclip_paddle_sweep_tasks with `values`"""
    T, Q, D = rows.T, rows.Q, rows.D
    c, entry, dim, P = _rows_call("tclip_paddle", rows, _capi.Problem(1, T, Q, K, rows.S, iters, 1, 0, 0), visual, values)
    u, v, w, preds = c.empty(*P, T, Q, K), c.empty(*P, T, K), c.empty(*P, T, K, D), c.empty(*P, T, Q, dtype=torch.int32)
    c.launch(entry, lambda ws, n, st: (*dim, *rows.args, _ptr(rows.y_s), *_swept(values, ctypes.c_float, lambd), _ptr(u),
                                       _ptr(v), _ptr(w), _ptr(preds), ws, n, st))
    return u, v, w, preds


def run_paddle(x_q, x_s, y_s, *, iters, lambd):
    """PADDLE: x_q (T,Q,K), x_s (T,S,K) f32 cuda, y_s (T,S) int64 cuda ->
    (u (T,Q,K), v (T,K), w (T,K,K), preds (T,Q) i32), cuda, not synchronised."""
    x_q = _query(x_q)
    x_s, y_s = _support(x_q, x_s, y_s)
    return _paddle(_dense_rows(x_q, x_s, y_s), x_q.shape[2], False, iters, lambd)


def run_paddle_visual(x_q, x_s, y_s, *, n_class, iters, lambd):
    """PADDLE on visual features: x_q (T,Q,D), x_s (T,S,D) raw embeddings f32 cuda, y_s (T,S) int64 cuda with labels in
    0..n_class-1 -> (u (T,Q,K), v (T,K), w (T,K,D), preds (T,Q) i32), cuda, not synchronised.  K = n_class cannot be read off a
    tensor shape here.  No text features: the reference's text-prompt u is dead (paddle.py:183-203)."""
    x_q = _query(x_q)
    x_s, y_s, K = _support_visual(x_q, x_s, y_s, n_class)
    return _paddle(_dense_rows(x_q, x_s, y_s), K, True, iters, lambd)


def run_paddle_tasks(table_q, q_idx, table_s, s_idx, y_s, cols=None, *, iters, lambd):
    """PADDLE fed from the task-batch loop's feature tables (tclip_paddle_run_tasks): table_q, table_s (rows,K) f32 cuda,
    q_idx (T,Q) / s_idx (T,S) rows of them, y_s (T,S) the re-indexed support labels, cols (T,K) the per-task column permutation
    of Tasks_Generator_few_shot.get_task or None -> (u (T,Q,K), v (T,K), w (T,K,K), preds (T,Q) i32), cuda, not synchronised.
    The support rows are read in place: no (T,S,K) tensor is built; the results are those of run_paddle on the materialised
    tensors, bit for bit."""
    K = table_q.shape[1]
    return _paddle(_task_tables(table_q, q_idx, table_s, s_idx, y_s, cols, K, "PADDLE"), K, False, iters, lambd)


def run_paddle_visual_tasks(table_q, q_idx, table_s, s_idx, y_s, *, n_class, iters, lambd):
    """PADDLE on visual features fed from the feature tables (tclip_paddle_visual_run_tasks): table_q, table_s (rows,D) raw
    embeddings f32 cuda with any D in 1..1024, q_idx (T,Q), s_idx (T,S), y_s (T,S) int64 labels in 0..n_class-1 as they are (no
    re-indexing and no column permutation on visual features) -> (u (T,Q,K), v (T,K), w (T,K,D), preds (T,Q) i32), cuda, not
    synchronised; the bits of run_paddle_visual on the materialised tensors."""
    K = _check_n_class(n_class)
    return _paddle(_task_tables(table_q, q_idx, table_s, s_idx, y_s, None, K, "PADDLE"), K, True, iters, lambd)


def sweep_paddle_tasks(table_q, q_idx, table_s, s_idx, y_s, cols=None, *, iters, values, n_class=None):
    """run_paddle_tasks (n_class=None) / run_paddle_visual_tasks (n_class given; cols must be None) for every lambd of `values`
    in one call (tclip_paddle_sweep_tasks) -> (u (P,T,Q,K), v (P,T,K), w (P,T,K,D), preds (P,T,Q) i32): slice i holds the
    bits of the single-value call with lambd = values[i].  The support class sums are taken once.  Not synchronised."""
    values = _sweep_values(values, "values")
    K, visual = _sweep_n_class(table_q, n_class, cols, "PADDLE")
    return _paddle(_task_tables(table_q, q_idx, table_s, s_idx, y_s, cols, K, "PADDLE"), K, visual, iters, None, values)


# ---- ALPHA_TIM and TIM_GD ------------------------------------------------------------------------------------------------------
ENTROPIES = {"Shannon": 0, "Alpha": 1}


def _check_entropies(entropies):
    for e in entropies:
        if e not in ENTROPIES:
            raise ValueError("Entropies must be in ['Shannon', 'Alpha']")        # tim.py:286, 295, 305


def _tim_params(lr, temp, alpha_value, loss_weights, entropies):
    return _capi.TimParams(float(lr), float(temp), float(alpha_value), (ctypes.c_float * 3)(*[float(w) for w in loss_weights]),
                           (ctypes.c_int32 * 3)(*[ENTROPIES[e] for e in entropies]))


def _check_n_batches(rows, n_batches):
    if rows.T % n_batches:
        raise ValueError("the number of tasks must be a multiple of n_batches")


def _alpha_tim(rows, K, visual, iters, temp, lr, alpha_value, loss_weights, entropies, n_batches, values=None):
    """ALPHA_TIM on rows of D elements: tclip_alpha_tim[_visual]_run[_tasks] with alpha_value, tclip_alpha_tim_sweep_tasks with
    `values` (the struct's alpha_value is not read there)"""
    _check_n_batches(rows, n_batches)
    T, Q, D = rows.T, rows.Q, rows.D
    prm = _tim_params(lr, temp, alpha_value if values is None else 0.0, loss_weights, entropies)
    c, entry, dim, P = _rows_call("tclip_alpha_tim", rows, _capi.Problem(n_batches, T // n_batches, Q, K, rows.S, iters, 1, 0, 0),
                                  visual, values)
    weights, logits_q = c.empty(*P, T, K, D), c.empty(*P, T, Q, K)
    preds, crit = c.empty(*P, T, Q, dtype=torch.int32), c.empty(*P, n_batches, iters)
    c.launch(entry, lambda ws, n, st: (*dim, ctypes.byref(prm), *rows.args, _ptr(rows.y_s), *_swept(values), _ptr(weights),
                                       _ptr(logits_q), _ptr(preds), _ptr(crit), ws, n, st))
    return weights, logits_q, preds, crit


def run_alpha_tim(x_q, x_s, y_s, *, iters, temp, lr, alpha_value, loss_weights=(1.0, 1.0, 1.0),
                  entropies=("Shannon", "Alpha", "Alpha"), n_batches=1):
    """ALPHA_TIM: x_q (T,Q,K), x_s (T,S,K) f32 cuda, y_s (T,S) int64 cuda -> (weights (T,K,K), logits_q (T,Q,K) of the
    last iteration's forward pass, preds (T,Q) i32 = their argmax, criterions (n_batches, iters)), cuda, not synchronised."""
    _check_entropies(entropies)
    x_q = _query(x_q)
    x_s, y_s = _support(x_q, x_s, y_s)
    return _alpha_tim(_dense_rows(x_q, x_s, y_s), x_q.shape[2], False, iters, temp, lr, alpha_value, loss_weights, entropies, n_batches)


def run_alpha_tim_visual(x_q, x_s, y_s, *, n_class, iters, temp, lr, alpha_value, loss_weights=(1.0, 1.0, 1.0),
                         entropies=("Shannon", "Alpha", "Alpha"), n_batches=1):
    """ALPHA_TIM on visual features: x_q (T,Q,D), x_s (T,S,D) raw embeddings f32 cuda with any D in 1..1024, y_s (T,S) int64 cuda
    with labels in 0..n_class-1 -> (weights (T,K,D), logits_q (T,Q,K) of the last iteration's forward pass, preds (T,Q) i32 =
    their argmax, criterions (n_batches, iters)), cuda, not synchronised.  K = n_class cannot be read off a tensor shape here."""
    _check_entropies(entropies)
    x_q = _query(x_q)
    if x_s.dim() != 3 or x_s.shape[1] < 1:
        raise ValueError("ALPHA_TIM is a few-shot method: x_s must be (T,S,D) with n_support = S positive")
    x_s, y_s, K = _support_visual(x_q, x_s, y_s, n_class)
    return _alpha_tim(_dense_rows(x_q, x_s, y_s), K, True, iters, temp, lr, alpha_value, loss_weights, entropies, n_batches)


def run_alpha_tim_tasks(table_q, q_idx, table_s, s_idx, y_s, cols=None, *, iters, temp, lr, alpha_value,
                        loss_weights=(1.0, 1.0, 1.0), entropies=("Shannon", "Alpha", "Alpha"), n_batches=1):
    """ALPHA_TIM fed from the task-batch loop's feature tables (tclip_alpha_tim_run_tasks): table_q, table_s (rows,K) f32 cuda,
    q_idx (T,Q) / s_idx (T,S) rows of them, y_s (T,S) the re-indexed support labels, cols (T,K) the per-task column permutation
    of Tasks_Generator_few_shot.get_task or None -> what run_alpha_tim returns on the materialised tensors, bit for bit; neither
    (T,S,K) nor (T,Q,K) is built: the table rows are read in place in every Adam step.  Not synchronised."""
    K = table_q.shape[1]
    _check_entropies(entropies)
    rows = _task_tables(table_q, q_idx, table_s, s_idx, y_s, cols, K, "ALPHA_TIM")
    return _alpha_tim(rows, K, False, iters, temp, lr, alpha_value, loss_weights, entropies, n_batches)


def run_alpha_tim_visual_tasks(table_q, q_idx, table_s, s_idx, y_s, *, n_class, iters, temp, lr, alpha_value,
                               loss_weights=(1.0, 1.0, 1.0), entropies=("Shannon", "Alpha", "Alpha"), n_batches=1):
    """ALPHA_TIM on visual features fed from the feature tables (tclip_alpha_tim_visual_run_tasks): tables (rows,D) with any D
    in 1..1024, y_s (T,S) int64 labels in 0..n_class-1 as they are, no column permutation -> the bits of run_alpha_tim_visual
    on the materialised tensors.  Not synchronised."""
    K = _check_n_class(n_class)
    _check_entropies(entropies)
    rows = _task_tables(table_q, q_idx, table_s, s_idx, y_s, None, K, "ALPHA_TIM")
    return _alpha_tim(rows, K, True, iters, temp, lr, alpha_value, loss_weights, entropies, n_batches)


def sweep_alpha_tim_tasks(table_q, q_idx, table_s, s_idx, y_s, cols=None, *, iters, temp, lr, values, loss_weights=(1.0, 1.0, 1.0),
                          entropies=("Shannon", "Alpha", "Alpha"), n_batches=1, n_class=None):
    """run_alpha_tim_tasks (n_class=None) / run_alpha_tim_visual_tasks (n_class given) for every alpha_value of `values` in one
    call (tclip_alpha_tim_sweep_tasks) -> (weights (P,T,K,D), logits_q (P,T,Q,K), preds (P,T,Q) i32, criterions
    (P,n_batches,iters)), slice i the bits of the single-value call with alpha_value = values[i].  The Adam loop runs over
    P * T solves in one set of launches per step; solve (i, t) reads the rows of task t in place.  Not synchronised."""
    values = _sweep_values(values, "values")
    _check_entropies(entropies)
    K, visual = _sweep_n_class(table_q, n_class, cols, "ALPHA_TIM")
    rows = _task_tables(table_q, q_idx, table_s, s_idx, y_s, cols, K, "ALPHA_TIM")
    return _alpha_tim(rows, K, visual, iters, temp, lr, None, loss_weights, entropies, n_batches, values)


def _tim_gd(rows, K, iters, temp, lr, loss_weights, n_batches):
    """TIM_GD on rows of D elements, D always passed: tclip_tim_gd_run[_tasks]"""
    _check_n_batches(rows, n_batches)
    T, Q, D = rows.T, rows.Q, rows.D
    lw = (ctypes.c_float * 3)(*[float(w) for w in loss_weights])
    c, entry, dim, _ = _rows_call("tclip_tim_gd", rows, _capi.Problem(n_batches, T // n_batches, Q, K, rows.S, iters, 1, 0, 0), True,
                                  infix="")
    weights, logits_q, preds, crit = c.empty(T, K, D), c.empty(T, Q, K), c.empty(T, Q, dtype=torch.int32), c.empty(iters, T)
    c.launch(entry, lambda ws, n, st: (*dim, ctypes.c_double(float(lr)), ctypes.c_float(float(temp)), lw, *rows.args, _ptr(rows.y_s),
                                       _ptr(weights), _ptr(logits_q), _ptr(preds), _ptr(crit), ws, n, st))
    return weights, logits_q, preds, crit


def run_tim_gd(x_q, x_s, y_s, *, n_class, iters, temp, lr, loss_weights=(1.0, 0.3, 1.0), n_batches=1):
    """TIM_GD on either feature kind: x_q (T,Q,D), x_s (T,S,D) f32 cuda with any D in 1..1024 (D = n_class: probability
    features), y_s (T,S) int64 cuda with labels in 0..n_class-1 -> (weights (T,K,D), logits_q (T,Q,K) of the last iteration's
    forward pass, preds (T,Q) i32 = their argmax, criterions (iters, T): one value per step and TASK), cuda, not synchronised.
    K = n_class cannot be read off a tensor shape here.  Tasks never interact, so n_batches only has to divide T."""
    x_q = _query(x_q)
    if x_s.dim() != 3 or x_s.shape[1] < 1:
        raise ValueError("TIM_GD is a few-shot method: x_s must be (T,S,D) with n_support = S positive")
    x_s, y_s, K = _support_visual(x_q, x_s, y_s, n_class)
    return _tim_gd(_dense_rows(x_q, x_s, y_s), K, iters, temp, lr, loss_weights, n_batches)


def run_tim_gd_tasks(table_q, q_idx, table_s, s_idx, y_s, cols=None, *, n_class, iters, temp, lr, loss_weights=(1.0, 0.3, 1.0),
                     n_batches=1):
    """TIM_GD on either feature kind fed from the feature tables (tclip_tim_gd_run_tasks): tables (rows,D) f32 cuda with any D in
    1..1024, q_idx (T,Q) / s_idx (T,S) rows of them, y_s (T,S) int64 labels in 0..n_class-1 (re-indexed on probability
    features), cols (T,D) the per-task column permutation on probability features (D = n_class) or None -> what run_tim_gd
    returns on the materialised tensors, bit for bit; the table rows are read in place in every Adam step.  Not synchronised."""
    K = _check_n_class(n_class)
    if cols is not None and table_q.dim() == 2 and table_q.shape[1] != K:
        raise ValueError("TIM_GD permutes columns on probability features only: cols needs tables of n_class columns")
    return _tim_gd(_task_tables(table_q, q_idx, table_s, s_idx, y_s, cols, K, "TIM_GD"), K, iters, temp, lr, loss_weights, n_batches)


# ---- LAPLACIAN_SHOT ------------------------------------------------------------------------------------------------------------
NORM_TYPES = {"UN": 0, "L2N": 1, "CL2N": 2}


def _check_lshot_norm(norm_type):
    if norm_type not in ("UN", "L2N"):
        raise ValueError("norm_type must be 'UN' or 'L2N' (the reference's CL2N needs a train mean it never passes)")


def _laplacian_shot(rows, K, visual, iters, knn, lmd, norm_type, values=None):
    """LAPLACIAN_SHOT on rows of D elements: tclip_laplacian_shot[_visual]_run[_tasks] with lmd, tclip_laplacian_shot_sweep_tasks
    with `values`; the unary term and the neighbours, which no lmd enters, have no leading P"""
    T, Q = rows.T, rows.Q
    c, entry, dim, P = _rows_call("tclip_laplacian_shot", rows, _capi.Problem(1, T, Q, K, rows.S, iters, 1, 0, 0), visual, values)
    unary, nbr = c.empty(T, Q, K), c.empty(T, Q, max(int(knn) - 1, 1), dtype=torch.int32)
    preds_iter, energies = c.empty(*P, T, max(iters, 1), Q, dtype=torch.int32), c.empty(*P, T, max(iters, 1), dtype=torch.float64)
    c.launch(entry, lambda ws, n, st: (*dim, *rows.args, _ptr(rows.y_s), ctypes.c_int32(int(knn)),
                                       *_swept(values, ctypes.c_double, lmd), ctypes.c_int32(NORM_TYPES[norm_type]),
                                       _ptr(unary), _ptr(nbr), _ptr(preds_iter), _ptr(energies), ws, n, st))
    return unary, nbr, preds_iter, energies


def run_laplacian_shot(x_q, x_s, y_s, *, iters, knn, lmd, norm_type="L2N"):
    """LAPLACIAN_SHOT: x_q (T,Q,K), x_s (T,S,K) f32 cuda, y_s (T,S) int64 cuda -> (unary (T,Q,K), neighbours (T,Q,knn-1) i32,
    preds_iter (T,iters,Q) i32, energies (T,iters) f64), cuda, not synchronised."""
    _check_lshot_norm(norm_type)
    x_q = _query(x_q)
    x_s, y_s = _support(x_q, x_s, y_s)
    return _laplacian_shot(_dense_rows(x_q, x_s, y_s), x_q.shape[2], False, iters, knn, lmd, norm_type)


def run_laplacian_shot_visual(x_q, x_s, y_s, *, n_class, iters, knn, lmd, norm_type="L2N"):
    """LAPLACIAN_SHOT on visual features: x_q (T,Q,D), x_s (T,S,D) raw embeddings f32 cuda with any D in 1..1024, y_s (T,S)
    int64 cuda with labels in 0..n_class-1 -> (unary (T,Q,K), neighbours (T,Q,knn-1) i32, preds_iter (T,iters,Q) i32, energies
    (T,iters) f64), cuda, not synchronised.  K = n_class cannot be read off a tensor shape here."""
    _check_lshot_norm(norm_type)
    x_q = _query(x_q)
    x_s, y_s, K = _support_visual(x_q, x_s, y_s, n_class)
    return _laplacian_shot(_dense_rows(x_q, x_s, y_s), K, True, iters, knn, lmd, norm_type)


def run_laplacian_shot_tasks(table_q, q_idx, table_s, s_idx, y_s, cols=None, *, iters, knn, lmd, norm_type="L2N"):
    """LAPLACIAN_SHOT fed from the task-batch loop's feature tables (tclip_laplacian_shot_run_tasks): table_q, table_s (rows,K)
    f32 cuda, q_idx (T,Q) / s_idx (T,S) rows of them, y_s (T,S) the re-indexed support labels, cols (T,K) the per-task column
    permutation of Tasks_Generator_few_shot.get_task or None -> what run_laplacian_shot returns on the materialised tensors,
    bit for bit; neither (T,S,K) nor (T,Q,K) is built.  Not synchronised."""
    K = table_q.shape[1]
    _check_lshot_norm(norm_type)
    rows = _task_tables(table_q, q_idx, table_s, s_idx, y_s, cols, K, "LAPLACIAN_SHOT")
    return _laplacian_shot(rows, K, False, iters, knn, lmd, norm_type)


def run_laplacian_shot_visual_tasks(table_q, q_idx, table_s, s_idx, y_s, *, n_class, iters, knn, lmd, norm_type="L2N"):
    """LAPLACIAN_SHOT on visual features fed from the feature tables (tclip_laplacian_shot_visual_run_tasks): tables (rows,D)
    with any D in 1..1024, y_s (T,S) int64 labels in 0..n_class-1 as they are, no column permutation -> the bits of
    run_laplacian_shot_visual on the materialised tensors.  Not synchronised."""
    K = _check_n_class(n_class)
    _check_lshot_norm(norm_type)
    rows = _task_tables(table_q, q_idx, table_s, s_idx, y_s, None, K, "LAPLACIAN_SHOT")
    return _laplacian_shot(rows, K, True, iters, knn, lmd, norm_type)


def sweep_laplacian_shot_tasks(table_q, q_idx, table_s, s_idx, y_s, cols=None, *, iters, knn, values, norm_type="L2N", n_class=None):
    """run_laplacian_shot_tasks (n_class=None) / run_laplacian_shot_visual_tasks (n_class given) for every lmd of `values` in one
    call (tclip_laplacian_shot_sweep_tasks) -> (unary (T,Q,K) and neighbours (T,Q,knn-1) i32, which no lmd enters, once;
    preds_iter (P,T,iters,Q) i32, energies (P,T,iters) f64, slice i the bits of the single-value call with lmd = values[i]).
    Normalisation, prototypes, unary term and kNN graph run once per task, the updates on a grid of (task, value).  Not
    synchronised."""
    values = _sweep_values(values, "values")
    _check_lshot_norm(norm_type)
    K, visual = _sweep_n_class(table_q, n_class, cols, "LAPLACIAN_SHOT")
    rows = _task_tables(table_q, q_idx, table_s, s_idx, y_s, cols, K, "LAPLACIAN_SHOT")
    return _laplacian_shot(rows, K, visual, iters, knn, None, norm_type, values)


def argmax_rows(x):
    """x (..., K) f32 cuda -> int32 (...) indices of the first maximum of every row, cuda, not synchronised."""
    _require_cuda(x, "x")
    x = x.contiguous().float()
    K = x.shape[-1]
    rows = x.numel() // K
    with torch.cuda.device(x.device):
        labels = torch.empty(x.shape[:-1], dtype=torch.int32, device=x.device)
        rc = _capi.lib().tclip_argmax_rows(_ptr(x), ctypes.c_int64(rows), ctypes.c_int32(K), _ptr(labels), _stream())
        _capi.check(rc, "tclip_argmax_rows")
    return labels


# ---- BD-CSPN -------------------------------------------------------------------------------------------------------------------
def _check_bdcspn_norm(norm_type):
    if norm_type not in NORM_TYPES:
        raise ValueError(f"norm_type must be one of {sorted(NORM_TYPES)}")


def _bdcspn(rows, K, visual, temp, norm_type, values=None):
    """BD-CSPN on rows of D elements: tclip_bdcspn[_visual]_run[_tasks] with temp, tclip_bdcspn_sweep_tasks with `values`"""
    T, Q, D = rows.T, rows.Q, rows.D
    c, entry, dim, P = _rows_call("tclip_bdcspn", rows, _capi.Problem(1, T, Q, K, rows.S, 1, 1, 0, 0), visual, values)
    prototypes, u, preds = c.empty(*P, T, K, D), c.empty(*P, T, Q, K), c.empty(*P, T, Q, dtype=torch.int32)
    c.launch(entry, lambda ws, n, st: (*dim, *rows.args, _ptr(rows.y_s), *_swept(values, ctypes.c_float, temp),
                                       ctypes.c_int32(NORM_TYPES[norm_type]), _ptr(prototypes), _ptr(u), _ptr(preds), ws, n, st))
    return prototypes, u, preds


def run_bdcspn(x_q, x_s, y_s, *, temp, norm_type="L2N"):
    """BD-CSPN: x_q (T,Q,K), x_s (T,S,K) f32 cuda, y_s (T,S) int64 cuda ->
    (prototypes (T,K,K), u (T,Q,K), preds (T,Q) i32), cuda, not synchronised."""
    _check_bdcspn_norm(norm_type)
    x_q = _query(x_q)
    x_s, y_s = _support(x_q, x_s, y_s)
    return _bdcspn(_dense_rows(x_q, x_s, y_s), x_q.shape[2], False, temp, norm_type)


def run_bdcspn_visual(x_q, x_s, y_s, *, n_class, temp, norm_type="L2N"):
    """BD-CSPN on visual features: x_q (T,Q,D), x_s (T,S,D) f32 cuda, y_s (T,S) int64 cuda with labels in 0..n_class-1 ->
    (rectified prototypes (T,K,D), u (T,Q,K), preds (T,Q) i32), cuda, not synchronised."""
    _check_bdcspn_norm(norm_type)
    x_q = _query(x_q)
    x_s, y_s, K = _support_visual(x_q, x_s, y_s, n_class)
    return _bdcspn(_dense_rows(x_q, x_s, y_s), K, True, temp, norm_type)


def run_bdcspn_tasks(table_q, q_idx, table_s, s_idx, y_s, cols=None, *, temp, norm_type="L2N"):
    """BD-CSPN fed from the task-batch loop's feature tables (tclip_bdcspn_run_tasks): table_q, table_s (rows,K) f32 cuda,
    q_idx (T,Q) / s_idx (T,S) rows of them, y_s (T,S) the re-indexed support labels, cols (T,K) the per-task column permutation
    of Tasks_Generator_few_shot.get_task or None -> (prototypes (T,K,K), u (T,Q,K), preds (T,Q) i32), cuda, not synchronised:
    the bits of run_bdcspn on the materialised tensors.  Neither (T,S,K) nor (T,Q,K) is built, and the workspace is smaller than
    the dense one by the normalised support rows (they share the logits' region)."""
    K = table_q.shape[1]
    _check_bdcspn_norm(norm_type)
    return _bdcspn(_task_tables(table_q, q_idx, table_s, s_idx, y_s, cols, K, "BDCSPN"), K, False, temp, norm_type)


def run_bdcspn_visual_tasks(table_q, q_idx, table_s, s_idx, y_s, *, n_class, temp, norm_type="L2N"):
    """BD-CSPN on visual features fed from the feature tables (tclip_bdcspn_visual_run_tasks): tables (rows,D) with any D in
    1..1024, y_s (T,S) int64 labels in 0..n_class-1 as they are, no column permutation -> (rectified prototypes (T,K,D),
    u (T,Q,K), preds (T,Q) i32): the bits of run_bdcspn_visual on the materialised tensors.  Not synchronised."""
    K = _check_n_class(n_class)
    _check_bdcspn_norm(norm_type)
    return _bdcspn(_task_tables(table_q, q_idx, table_s, s_idx, y_s, None, K, "BDCSPN"), K, True, temp, norm_type)


def sweep_bdcspn_tasks(table_q, q_idx, table_s, s_idx, y_s, cols=None, *, values, norm_type="L2N", n_class=None):
    """run_bdcspn_tasks (n_class=None) / run_bdcspn_visual_tasks (n_class given) for every temp of `values` in one call
    (tclip_bdcspn_sweep_tasks) -> (prototypes (P,T,K,D), u (P,T,Q,K), preds (P,T,Q) i32), slice i the bits of the single-value
    call with temp = values[i].  Everything up to the augmented set runs once.  Not synchronised."""
    values = _sweep_values(values, "values")
    _check_bdcspn_norm(norm_type)
    K, visual = _sweep_n_class(table_q, n_class, cols, "BDCSPN")
    return _bdcspn(_task_tables(table_q, q_idx, table_s, s_idx, y_s, cols, K, "BDCSPN"), K, visual, None, norm_type, values)


MATCHING = ("host", "device")


def _check_matching(matching):
    if matching not in MATCHING:
        raise ValueError(f"matching must be one of {MATCHING}, got {matching!r}")
    return _match_device if matching == "device" else _match


def clustering_accuracy(x_q, preds, y_q, graph_matching=True, *, matching="host"):
    """Zero-shot accuracy tail: device prototypes of the predicted clusters, then the assignment of clusters to classes.

    x_q (T,Q,K) cuda f32, preds (T,Q) cuda i32, y_q (T,Q) int64 (any device).
    matching="host" (the default): the assignment runs on host threads; the call synchronises the stream and returns
    (acc (T,) f32 cpu, new_preds (T,Q) i32 cpu).
    matching="device": tclip_match_clusters on the current stream, the same bits; returns (acc, new_preds) on the device,
    not synchronised.  A task the host path would raise RuntimeError for has acc = NaN there (match_status_ok)."""
    match = _check_matching(matching)
    _require_cuda(x_q, "x_q")
    x_q = x_q.contiguous().float()
    T, Q, K = x_q.shape
    dev = x_q.device
    lib = _capi.lib()
    cmax = min(Q, K)
    with torch.cuda.device(dev):
        ws_bytes = lib.tclip_prototype_workspace_bytes(T, Q, K)
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=dev)
        off = (-ws.data_ptr()) % 256
        n_clusters = torch.empty(T, dtype=torch.int32, device=dev)
        ids = torch.empty(T, cmax, dtype=torch.int32, device=dev)
        protos = torch.empty(T, cmax, K, device=dev)        # rows beyond a task's cluster count are never read
        preds = preds.to(dev).int().contiguous()
        rc = lib.tclip_cluster_prototypes(T, Q, K, _ptr(x_q), _ptr(preds), _ptr(n_clusters), _ptr(ids), _ptr(protos),
                                          ctypes.c_void_p(ws.data_ptr() + off), ws_bytes, _stream())
        _capi.check(rc, "tclip_cluster_prototypes")
    return match(lib, T, Q, K, preds, n_clusters, ids, protos, y_q, graph_matching, cmax, dev)


VISUAL_METHODS = {"soft_kmeans": 0, "hard_kmeans": 1, "em_gaussian": 2}     # TCLIP_VISUAL_* of include/tclip.h


def visual_init(x_q, text, T):
    """The visual k-means / CLIP initialisation (soft_kmeans.py:185-197): u0[t] = softmax_k(T * (x_q[t]/||x_q[t]|| @ text.T)),
    the scale after the dot product.  x_q (..., D) f32 cuda raw embeddings, text (K, D) unit-norm text features ->
    (..., K) f32 cuda, not synchronised (tclip_visual_init)."""
    _require_cuda(x_q, "x_q")
    x_q = x_q.contiguous().float()
    text = text.to(x_q.device).contiguous().float()
    D = x_q.shape[-1]
    if text.dim() != 2 or text.shape[1] != D:
        raise ValueError(f"text features must be (K, {D}) for {D}-dim embeddings, got {tuple(text.shape)}")
    K = text.shape[0]
    rows = x_q.numel() // D
    out = torch.empty(*x_q.shape[:-1], K, device=x_q.device)
    with torch.cuda.device(x_q.device):
        rc = _capi.lib().tclip_visual_init(_ptr(x_q), _ptr(text), ctypes.c_int64(rows), ctypes.c_int32(D), ctypes.c_int32(K),
                                           ctypes.c_float(float(T)), _ptr(out), _stream())
    _capi.check(rc, "tclip_visual_init")
    return out


def _run_visual(method, x_q, u0, iters, temperature, lambd=0, n_batches=1):
    x_q = _query(x_q)
    _require_cuda(u0, "u0")
    u0 = u0.to(x_q.device).contiguous().float()
    T, Q, D = x_q.shape
    if u0.dim() != 3 or u0.shape[0] != T or u0.shape[1] != Q:
        raise ValueError("u0 must be (T,Q,K) with the T and Q of x_q")
    K = u0.shape[2]
    c, u, w, preds = _kmeans_call(x_q, K, "tclip_visual_workspace_bytes", ctypes.c_int32(D), iters=iters, lambd=lambd,
                                  n_batches=n_batches)
    hard, emg = method == "hard_kmeans", method == "em_gaussian"
    v = c.empty(T, K) if emg else None
    crit = c.empty(n_batches, max(iters, 1))[:, :iters].contiguous() if hard else None
    c.launch("tclip_kmeans_visual_run", lambda ws, n, st: (ctypes.c_int32(D), ctypes.c_int32(VISUAL_METHODS[method]), _ptr(x_q),
                                                           _ptr(u0), ctypes.c_float(float(temperature)), _ptr(u), _ptr(v), _ptr(w),
                                                           _ptr(preds), _ptr(crit), ws, n, st))
    return u, v, w, preds, crit


def run_soft_kmeans_visual(x_q, u0, *, iters, temperature):
    """SOFT_KMEANS on visual features: x_q (T,Q,D) raw embeddings, u0 (T,Q,K) the initial responsibilities (visual_init) ->
    (u (T,Q,K), w (T,K,D), preds (T,Q) i32), cuda, not synchronised."""
    u, _, w, preds, _ = _run_visual("soft_kmeans", x_q, u0, iters, temperature)
    return u, w, preds


def run_hard_kmeans_visual(x_q, u0, *, iters, n_batches=1):
    """HARD_KMEANS on visual features -> (u one-hot (T,Q,K), w (T,K,D), preds (T,Q) i32, criterions (n_batches, iters)), cuda,
    not synchronised.  The reference's HARD_KMEANS loop has no temperature."""
    u, _, w, preds, crit = _run_visual("hard_kmeans", x_q, u0, iters, 1.0, n_batches=n_batches)
    return u, w, preds, crit


def run_em_gaussian_visual(x_q, u0, *, iters, temperature, lambd):
    """EM_GAUSSIAN on visual features -> (u (T,Q,K), v (T,K), w (T,K,D), preds (T,Q) i32), cuda, not synchronised."""
    u, v, w, preds, _ = _run_visual("em_gaussian", x_q, u0, iters, temperature, lambd=lambd)
    return u, v, w, preds


def run_em_gaussian_cov_visual(x_q, u0, *, iters, lambd):
    """EM_GAUSSIAN_COV on visual features: x_q (T,Q,D) raw embeddings, D <= 1024, u0 (T,Q,K) the initial responsibilities
    (visual_init) -> (u (T,Q,K), v (T,K), w (T,K,D), s (T,K,D), preds (T,Q) i32), cuda, not synchronised.  Accuracy:
    clustering_accuracy_visual."""
    if x_q.dim() != 3:
        raise ValueError("x_q must be (T,Q,D)")
    T, Q, D = x_q.shape
    if u0.dim() != 3 or u0.shape[0] != T or u0.shape[1] != Q:
        raise ValueError("u0 must be (T,Q,K) with the T and Q of x_q")
    if D > 1024:
        raise ValueError(f"embeddings of at most 1024 elements, got {D}")
    for t, name in ((x_q, "x_q"), (u0, "u0")):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a cuda tensor: the engine has no CPU path")
    x_q = _query(x_q)
    u0 = u0.to(x_q.device).contiguous().float()
    K = u0.shape[2]
    c, u, w, preds = _kmeans_call(x_q, K, "tclip_em_gaussian_cov_visual_workspace_bytes", ctypes.c_int32(D), iters=iters, lambd=lambd)
    v, s = c.empty(T, K), c.empty(T, K, D)
    c.launch("tclip_em_gaussian_cov_visual_run", lambda ws, n, st: (ctypes.c_int32(D), _ptr(x_q), _ptr(u0), _ptr(u), _ptr(v), _ptr(w),
                                                                    _ptr(s), _ptr(preds), ws, n, st))
    return u, v, w, s, preds


def _match(lib, T, Q, K, preds, n_clusters, ids, rows, y_q, graph_matching, cmax, dev):
    """host half of the accuracy tail: copies the rows of the fullest task to the host and matches clusters to classes"""
    preds_h, nc_h = preds.cpu(), n_clusters.cpu()
    used = max(1, min(cmax, int(nc_h.max())))
    ids_h = torch.empty((T, used), dtype=torch.int32, pin_memory=True)
    rows_h = torch.empty((T, used, K), dtype=torch.float32, pin_memory=True)
    with torch.cuda.device(dev):
        ids_h.copy_(ids[:, :used], non_blocking=True)
        rows_h.copy_(rows[:, :used], non_blocking=True)
        torch.cuda.current_stream().synchronize()
    y_h = y_q.reshape(T, Q).long().cpu().contiguous()
    new_preds = torch.empty(T, Q, dtype=torch.int32)
    acc = torch.empty(T, dtype=torch.float32)
    rc = lib.tclip_match_clusters_host_strided(T, Q, K, _ptr(preds_h), _ptr(nc_h), _ptr(ids_h), _ptr(rows_h), _ptr(y_h),
                                               int(bool(graph_matching)), used, _ptr(new_preds), _ptr(acc))
    _capi.check(rc, "tclip_match_clusters_host_strided")
    return acc, new_preds


def _match_device(lib, T, Q, K, preds, n_clusters, ids, rows, y_q, graph_matching, cmax, dev):
    """the matching on the device (tclip_match_clusters) from the full (T, cmax, K) rows: nothing is copied to the host or
    read back and the stream is not synchronised; a failed task has acc = NaN and new_preds = -1"""
    with torch.cuda.device(dev):
        y_d = y_q.reshape(T, Q).to(dev).long().contiguous()
        new_preds = torch.empty(T, Q, dtype=torch.int32, device=dev)
        acc = torch.empty(T, dtype=torch.float32, device=dev)
        status = torch.empty(T, dtype=torch.int32, device=dev)
        ws_bytes = lib.tclip_match_clusters_workspace_bytes(T, Q, K, cmax)
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=dev) if ws_bytes else None
        ws_ptr = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256) if ws_bytes else None
        rc = lib.tclip_match_clusters(T, Q, K, _ptr(preds), _ptr(n_clusters), _ptr(ids), _ptr(rows), _ptr(y_d),
                                      int(bool(graph_matching)), cmax, _ptr(new_preds), _ptr(acc), _ptr(status), ws_ptr, ws_bytes,
                                      _stream())
        _capi.check(rc, "tclip_match_clusters")
    return acc, new_preds


def match_status_ok(acc):
    """For callers of matching="device" once they bring the accuracies to the host: raises the RuntimeError the host path
    raises when a task could not be matched (a label outside 0..K-1, an infeasible assignment, e.g. a NaN prototype row) -
    such a task's accuracy is NaN - and names the tasks.  Returns `acc` on the CPU.  Copying from the device waits for it."""
    acc = acc.detach().cpu()
    failed = torch.nonzero(torch.isnan(acc.reshape(acc.shape[0], -1)).any(1)).flatten().tolist() if acc.numel() else []
    if failed:
        raise RuntimeError(f"tclip_match_clusters failed for task(s) {failed}: a cluster id or prediction outside 0..K-1, "
                           "or no feasible assignment (NaN prototypes)")
    return acc


def clustering_accuracy_visual(x_q, preds, y_q, text, T, graph_matching=True, *, matching="host"):
    """Accuracy tail of the visual k-means methods (soft_kmeans.py:36-66): D-dim prototypes of the predicted clusters
    (tclip_cluster_prototypes_visual), probs = softmax_k(T * (p/||p||) . text_k) of each (tclip_probability_features: the
    scale before the dot product, as the reference's tail has it), host matching of clusters to classes on those rows.
    x_q (T,Q,D) cuda f32, preds (T,Q) cuda i32, y_q (T,Q) int64, text (K,D).  Returns (acc (T,) f32 cpu, new_preds (T,Q) i32 cpu);
    with matching="device" the matching runs on the device too (tclip_match_clusters) and both come back on the device, not
    synchronised (see clustering_accuracy)."""
    match = _check_matching(matching)
    _require_cuda(x_q, "x_q")
    x_q = x_q.contiguous().float()
    n_task, Q, D = x_q.shape
    dev = x_q.device
    text = text.to(dev).contiguous().float()
    if text.dim() != 2 or text.shape[1] != D:
        raise ValueError(f"text features must be (K, {D}) for {D}-dim embeddings, got {tuple(text.shape)}")
    K = text.shape[0]
    lib = _capi.lib()
    cmax = min(Q, K)
    with torch.cuda.device(dev):
        preds = preds.to(dev).int().contiguous()
        n_clusters = torch.empty(n_task, dtype=torch.int32, device=dev)
        ids = torch.empty(n_task, cmax, dtype=torch.int32, device=dev)
        protos = torch.ones(n_task, cmax, D, device=dev)      # rows beyond a task's cluster count are scored but never read
        rc = lib.tclip_cluster_prototypes_visual(n_task, Q, K, D, _ptr(x_q), _ptr(preds), _ptr(n_clusters), _ptr(ids), _ptr(protos),
                                                 _stream())
        _capi.check(rc, "tclip_cluster_prototypes_visual")
        probs = torch.empty(n_task, cmax, K, device=dev)
        rc = lib.tclip_probability_features(_ptr(protos), _ptr(text), ctypes.c_int64(n_task * cmax), ctypes.c_int32(D),
                                            ctypes.c_int32(K), ctypes.c_float(float(T)), _ptr(probs), _stream())
        _capi.check(rc, "tclip_probability_features")
    return match(lib, n_task, Q, K, preds, n_clusters, ids, probs, y_q, graph_matching, cmax, dev)


def gather_rows(table, idx):
    """table (n,K) cuda f32, idx (m,) int64 -> (m,K) cuda f32 (device-side task construction)."""
    _require_cuda(table, "table")
    table = table.contiguous().float()
    idx = _index_tensor(idx.reshape(-1), table.shape[0], table.device, "idx")
    out = torch.empty(idx.numel(), table.shape[1], device=table.device)
    with torch.cuda.device(table.device):
        rc = _capi.lib().tclip_gather_rows(_ptr(table), table.shape[0], table.shape[1], _ptr(idx), idx.numel(), _ptr(out), _stream())
    _capi.check(rc, "tclip_gather_rows")
    return out


def debug_set_probe_chunks(chunks=-1):
    """Test hook: run the dead rows' limit-cycle probe after the first `chunks` chunks (0 = never,
    negative = default).  Results do not depend on it."""
    _capi.check(_capi.lib().tclip_debug_set_probe_chunks(int(chunks)), "tclip_debug_set_probe_chunks")


def debug_set_dead_head(iterations=-1):
    """Test hook: MM iterations a freshly dead row runs before the early limit-cycle probe (0 = no early probe: the whole first
    chunk, then the probe; negative = default).  Results do not depend on it."""
    _capi.check(_capi.lib().tclip_debug_set_dead_head(int(iterations)), "tclip_debug_set_dead_head")


def debug_set_rowset_min_rows(rows=-1):
    """Test hook: 0 forces the 32-lanes-per-row layout of the MM kernels for every row length (short rows
    normally use 8 or 16 lanes per row), negative restores the default rule.  Results do not depend on it."""
    _capi.check(_capi.lib().tclip_debug_set_rowset_min_rows(int(rows)), "tclip_debug_set_rowset_min_rows")


def profile_enable(on=True):
    _capi.check(_capi.lib().tclip_profile_enable(int(bool(on))), "tclip_profile_enable")


def profile_collect():
    """(mm_busy_ms, mm_launch_ms_sum, mm_launches, element_updates) since the last call;
    synchronises the device."""
    busy, total, n, upd = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _capi.check(_capi.lib().tclip_profile_collect(ctypes.byref(busy), ctypes.byref(total), ctypes.byref(n),
                                                  ctypes.byref(upd)), "tclip_profile_collect")
    return busy.value, total.value, n.value, upd.value


def profile_last_kernels():
    """{'k_mm_live': (busy_ms, launch_ms_sum, launches, element_updates), 'k_mm_split': (...)} of the last profile_collect()"""
    busy, total = (ctypes.c_double * 2)(), (ctypes.c_double * 2)()
    n, upd = (ctypes.c_int64 * 2)(), (ctypes.c_int64 * 2)()
    _capi.check(_capi.lib().tclip_profile_last_kernels(busy, total, n, upd), "tclip_profile_last_kernels")
    return {name: (busy[i], total[i], n[i], upd[i]) for i, name in enumerate(("k_mm_live", "k_mm_split"))}


def profile_last_split_sorts():
    """(wavefront-iterations k_mm_split ran, full placements among them) of the last profile_collect(): the kernel keeps
    the placement of its elements in the class queues across MM iterations and sorts anew only when one has left its class"""
    it, so = ctypes.c_int64(0), ctypes.c_int64(0)
    _capi.check(_capi.lib().tclip_profile_last_split_sorts(ctypes.byref(it), ctypes.byref(so)), "tclip_profile_last_split_sorts")
    return it.value, so.value
