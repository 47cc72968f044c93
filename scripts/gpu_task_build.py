"""Task construction alone at K = 1000, 4 shots, 100 tasks (softmax features): the fused builder against gather_rows +
relabel_batch.  Each route in groups of its own (empty allocator cache, one warm-up call, five timed calls), the groups
alternated twice: the caching allocator is in its own steady state for either route.  Host clock around a synchronise, and device
events around the same call."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "transductive-clip_amd"), os.path.join(ROOT, "transductive-clip_amd", "drop_in")):
    sys.path.insert(0, p)
import torch
from src.eval_few_shot import relabel_batch, relabel_indices
from tclip_amd import engine

DEV = torch.device("cuda", 0)
K, shots, T, Q, rows_per_class = 1000, 4, 100, 75, 20
S = K * shots
gen = torch.Generator().manual_seed(5)
labels = torch.arange(K).repeat_interleave(rows_per_class)
tab_s = torch.rand(K * rows_per_class, K, generator=gen).to(DEV)
tab_q = torch.rand(K * rows_per_class, K, generator=gen).to(DEV)
per_class = torch.arange(K * rows_per_class).view(K, rows_per_class)
si = torch.stack([per_class[:, torch.randperm(rows_per_class, generator=gen)[:shots]].reshape(-1) for _ in range(T)])
qi = torch.randint(0, K * rows_per_class, (T, Q), generator=gen)
y_s, y_q = labels[si.reshape(-1)].view(T, S), labels[qi.reshape(-1)].view(T, Q)


def builder():
    cols, a, b = relabel_indices(y_s, y_q, K)
    return engine.gather_task_rows(tab_s, si, cols), engine.gather_task_rows(tab_q, qi, cols), a, b


def host_route():
    x_s = engine.gather_rows(tab_s, si.reshape(-1)).view(-1, S, K)
    x_q = engine.gather_rows(tab_q, qi.reshape(-1)).view(-1, Q, K)
    return relabel_batch(x_s, x_q, y_s, y_q, True)


def one(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return wall, e0.elapsed_time(e1) / 1e3, torch.cuda.max_memory_allocated() - base, out


res = {"builder": [], "gather_rows_relabel_batch": []}
ref = [t.cpu() for t in builder()]
for rnd in range(2):
    for name, fn in (("builder", builder), ("gather_rows_relabel_batch", host_route)):
        torch.cuda.empty_cache()
        out = one(fn)[3]
        assert all(torch.equal(a, b.cpu()) for a, b in zip(ref, out))
        del out
        for rep in range(5):
            wall, dev_s, peak, out = one(fn)
            del out
            res[name].append({"wall_s": wall, "device_event_s": dev_s, "peak_bytes": peak})
            print(rnd, name, rep, f"wall {wall * 1e3:.2f} ms  events {dev_s * 1e3:.2f} ms  peak {peak / 1e6:.1f} MB", flush=True)
if len(sys.argv) > 1:      # optional: a file that receives the record
    json.dump(res, open(sys.argv[1], "w"), indent=1)
print(json.dumps(res))
