"""GPU: the hand-derived gradient of TIM_GD and ALPHA_TIM (csrc/tclip_tim.inc: k_tim_softmax, k_tim_marginal, k_tim_grad, the dW
GEMM with its column sums, k_tim_adam's first step) against the float64 autograd gradient of the restated loss, read out of ONE
Adam step through the public entries (tests/helpers/tim_probe.py), at the register-slot, tile and depth-slice edges up to 1024.

Per case: g64 = float64 autograd gradient at the class means, e(gpu) from the probe on the engine, e(ref32) from the probe on the
fp32 torch restatement, e(x) = max over the measured elements of |x - g64| / max(|g64|, 1e-3 max|g64| of the task).
  - on the restatement alone (host_side): with each of the three loss weights times 1.01 in turn the float64 gradient of THIS case
    has e >= 10 C e(ref32): the bound sees one per cent of every term at these inputs.  For that the loss weights of a case
    balance the three terms' largest gradient elements (tim_probe.balanced_weights) and each case has its own temperature;
  - at least 99 % of the elements are measured;
  - e(gpu) <= C e(ref32); and C e(ref32) < tim_probe.MUTATION_FLOOR / 10 (tests/test_tim_gradient_probe.py);
  - the logits of the same call (the forward pass at the class means) are within 2 x the fp32 restatement's own distance from
    the float64 one (prob_shapes.rel_err), and preds is the first-maximum argmax of the returned logits;
  - at three shapes the in-place entries give the weights of the dense ones bit for bit, at all 15 scales of the ladder.
The target is always the restatement, never an engine output.

C = 3.  Measured on MI355X, e(gpu) / e(ref32) of the gradient over the cases of a method: TIM_GD 0.05 .. 1.52, ALPHA_TIM
0.43 .. 2.08; two cases are above 2, both AAA at alpha 7: rows (D, K, S, Q) = (5, 3, 3, 1) 2.08 (e(gpu) 4.2e-06 against
2.0e-06: thirty elements, both a few ulp) and (16, 10, 40, 74) 2.02.  The closed-form gradient evaluated in float64 on the host
agrees with autograd to 1e-13, and in fp32 with torch's own sums it lands between 0.5 and 2.3 x the fp32 autograd error:
rounding in another operation order, no error, hence the largest ratio rounded up.  C e(ref32) is at most 3.8e-03 against
MUTATION_FLOOR / 10 = 8e-03; the smallest 1 % figure of a case over its 10 C e(ref32) is 4.4 (TIM_GD, K = 961, Q = 1, where
the two entropy terms cancel and the cross-entropy stands alone).  The logits: 0.17 .. 1.66.
What this test found and the kernels now avoid: with one accumulator over the whole contraction in
k_tim_gemm_mfma, gradient ratios of 6.1 to 11.8 at K = 960 .. 1024 on probability features and logits ratios up to 25; with
k_tim_marginal's sequential fp32 sum, 7.8 on AAA7 K = 65 Q = 128, 4.0 on AAA7 rows (16, 10, 40, 74), 3.3 on SAA2 K = 1023 Q = 128.
"""
import pytest
import torch

from helpers import tim_probe
from helpers.prob_shapes import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 3.0
QS = (1, 74, 75, 76, 77, 128)
ENTS = tuple(tim_probe.ENTROPIES)

# A case: (entropy setting of tim_probe.ENTROPIES or None for TIM_GD, probability features, D, K, shots, Q, T, temp).  The loss
# weights of a case are tim_probe.balanced_weights of its three float64 term gradients, and temp is the one of 15, 8, 5, 3 at
# which, on the restatement alone, a 1 % change of EVERY loss weight moves e furthest above 10 C e(ref32) (host_side asserts that
# it does): at temp 15 a one-shot support row sits on its own class mean with probability 1 and the cross-entropy term vanishes,
# and the reference's fp32 Alpha cross-entropy at alpha = 7 is 0 * inf (tim_probe.ENTROPIES).
# Probability features (D = K): K on both sides of the first 64-lane register slot of k_tim_softmax / k_tim_grad, around 512,
# the last slot empty (960) and holding one element (961), a ragged last slot (1000, 1023) and the full 16 (1024)
PROB_K = (63, 64, 65, 511, 513, 960, 961, 1000, 1023, 1024)
PROB_CASES = [
    (None, True, 63, 63, 1, 1, 9, 5.0), (None, True, 64, 64, 2, 74, 2, 15.0), (None, True, 65, 65, 1, 75, 3, 15.0),
    (None, True, 511, 511, 1, 76, 1, 15.0), (None, True, 513, 513, 1, 77, 1, 15.0), (None, True, 960, 960, 1, 128, 1, 5.0),
    (None, True, 961, 961, 1, 1, 1, 3.0), (None, True, 1000, 1000, 1, 74, 1, 5.0), (None, True, 1023, 1023, 1, 75, 1, 15.0),
    (None, True, 1024, 1024, 1, 76, 1, 15.0),
    ("AAA7", True, 63, 63, 1, 76, 2, 8.0), ("AAA7", True, 64, 64, 1, 77, 3, 5.0), ("AAA7", True, 65, 65, 2, 128, 1, 5.0),
    ("ASS05", True, 511, 511, 1, 74, 1, 15.0), ("SSS", True, 513, 513, 1, 75, 1, 5.0), ("SAA2", True, 960, 960, 1, 75, 1, 3.0),
    ("SSS", True, 961, 961, 1, 76, 1, 5.0), ("ASS05", True, 1000, 1000, 1, 77, 1, 15.0), ("SAA2", True, 1023, 1023, 1, 128, 1, 3.0),
    ("SAA2", True, 1024, 1024, 1, 1, 1, 3.0)]
# Rows of D elements, (D, K, S, Q): R = S + Q = 4, one partial depth-16 slice; a small case; one past a depth and a tile
# boundary; every tile interior with the 128-bit loads and R a multiple of 16; interior tiles on the 128-bit loads with a partial
# last slice of R; D > K and ragged everywhere; rows that are no multiple of 4; 1024
ROW_SHAPES = [(5, 3, 3, 1), (16, 10, 40, 74), (33, 65, 65, 76), (64, 64, 64, 64), (96, 128, 128, 77), (130, 37, 74, 75),
              (1023, 5, 5, 75), (1024, 6, 12, 77)]
# AAA7 where the class count is small: p^6 of the entropy terms is then within reach of the cross-entropy's p^-7
ROW_CASES = [
    (None, False, 5, 3, 1, 1, 1, 3.0), (None, False, 16, 10, 4, 74, 2, 15.0), (None, False, 33, 65, 1, 76, 3, 3.0),
    (None, False, 64, 64, 1, 64, 1, 15.0), (None, False, 96, 128, 1, 77, 2, 5.0), (None, False, 130, 37, 2, 75, 3, 15.0),
    (None, False, 1023, 5, 1, 75, 1, 5.0), (None, False, 1024, 6, 2, 77, 2, 5.0),
    ("AAA7", False, 5, 3, 1, 1, 2, 3.0), ("AAA7", False, 16, 10, 4, 74, 3, 5.0), ("SSS", False, 33, 65, 1, 76, 1, 3.0),
    ("ASS05", False, 64, 64, 1, 64, 2, 5.0), ("SAA2", False, 96, 128, 1, 77, 3, 5.0), ("SSS", False, 130, 37, 2, 75, 1, 5.0),
    ("AAA7", False, 1023, 5, 1, 75, 2, 8.0), ("AAA7", False, 1024, 6, 2, 77, 3, 8.0)]
CASES = PROB_CASES + ROW_CASES


def case_id(c):
    return "{}_{}_D{}_K{}_s{}_Q{}_T{}_temp{:g}".format(c[0] or "GD", "prob" if c[1] else "rows", *c[2:])


def test_cases_cover_what_they_claim():
    for gd in (True, False):
        mine = [c for c in CASES if (c[0] is None) == gd]
        assert {c[3] for c in mine if c[1]} == set(PROB_K) and all(c[2] == c[3] for c in mine if c[1])
        assert {(c[2], c[3], c[3] * c[4], c[5]) for c in mine if not c[1]} == set(ROW_SHAPES)
        assert {c[5] for c in mine if c[1]} == set(QS)
        assert all(1 <= c[6] <= 3 or c[6] == 9 for c in mine)
    assert any(c[6] == 9 for c in CASES) and {c[6] for c in CASES} >= {1, 2, 3}
    for e in ENTS:
        assert len({c[2:6] for c in CASES if c[0] == e}) >= 3, e
    # the conditions the row shapes are named for (kTimMfmaDepth = 16, kTimTile = 64)
    r = [s + q for _, _, s, q in ROW_SHAPES]
    assert r[0] < 16 and r[3] % 16 == 0 and all(x % 64 == 0 for x in ROW_SHAPES[3][:2])
    assert r[4] % 16 and all(x % 4 == 0 and x >= 64 for x in ROW_SHAPES[4][:2])
    assert ROW_SHAPES[2][0] == 33 and ROW_SHAPES[2][1] == 65 and ROW_SHAPES[6][0] % 4 and ROW_SHAPES[7][0] == 1024
    assert len(CASES) == len(set(CASES))


_HOST = {}


def host_side(case):
    """the inputs, g64, the fp32 restatement's probe and both forward passes of a case, made once and shared (never modified)"""
    if case not in _HOST:
        ent, prob, D, K, shots, Q, T, temp = case
        x_q, x_s, y_s = tim_probe.make_inputs(prob, D, K, shots, Q, T)
        prm, grad, run32 = tim_probe.restatement(ent, x_q, x_s, y_s, K, temp=temp)
        terms = tim_probe.term_gradients(grad)
        prm["loss_weights"] = tim_probe.balanced_weights(terms)
        g64, mutated = tim_probe.mutation_errors(terms, prm["loss_weights"])
        w0, _, lq64 = grad(torch.float64, prm["loss_weights"])
        assert bool(torch.isfinite(g64).all())
        g32, measured32 = tim_probe.probe(run32, prm["loss_weights"], w0, g64)
        e_ref32 = tim_probe.error(g32, g64, measured32)
        # a condition on the inputs, met by the restatement alone: the bound sees one per cent of every term of this case
        assert e_ref32 > 0 and min(mutated) >= 10 * C * e_ref32, (case_id(case), mutated, e_ref32)
        _HOST[case] = dict(x_q=x_q, x_s=x_s, y_s=y_s, prm=prm, w0=w0, g64=g64, lq64=lq64, lq32=grad(torch.float32, prm["loss_weights"])[2],
                           e_ref32=e_ref32, left_out32=tim_probe.share_left_out(measured32), mutated=mutated)
    return _HOST[case]


def engine_entry(case, tasks=False):
    """-> (the public entry of the case, its fixed keyword arguments)"""
    from tclip_amd import engine
    ent, prob, _, K, *_ = case
    kw = dict({k: v for k, v in host_side(case)["prm"].items() if k != "loss_weights"}, iters=1, lr=1.0)
    if ent is None:
        return (engine.run_tim_gd_tasks if tasks else engine.run_tim_gd), dict(kw, n_class=K)
    if prob:
        return (engine.run_alpha_tim_tasks if tasks else engine.run_alpha_tim), kw
    return (engine.run_alpha_tim_visual_tasks if tasks else engine.run_alpha_tim_visual), dict(kw, n_class=K)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gradient_and_forward_pass_against_float64(case):
    h = host_side(case)
    entry, kw = engine_entry(case)
    x_q, x_s, y_s = h["x_q"].to(DEV), h["x_s"].to(DEV), h["y_s"].to(DEV)
    forward = []

    def run(loss_weights):
        w, lq, preds, _ = entry(x_q, x_s, y_s, loss_weights=loss_weights, **kw)
        if not forward:
            forward.extend((lq.cpu(), preds.cpu()))
        return w

    g, measured = tim_probe.probe(run, h["prm"]["loss_weights"], h["w0"], h["g64"])
    torch.cuda.synchronize()
    left_out, e_gpu, e_ref32 = tim_probe.share_left_out(measured), tim_probe.error(g, h["g64"], measured), h["e_ref32"]
    lq, preds = forward
    l_gpu, l_ref32 = rel_err(lq, h["lq64"]), rel_err(h["lq32"], h["lq64"])
    print(f"{case_id(case)}: gradient e(gpu) {e_gpu:.3e} e(ref32) {e_ref32:.3e} ratio {e_gpu / e_ref32:.2f} left out {left_out:.4f} "
          f"(ref32 {h['left_out32']:.4f}) weights {h['prm']['loss_weights']} 1 % of a term {min(h['mutated']):.1e}; logits e(gpu) {l_gpu:.3e} e(ref32) {l_ref32:.3e} ratio {l_gpu / l_ref32:.2f}")
    assert h["left_out32"] <= 0.01 and left_out <= 0.01
    assert C * e_ref32 < tim_probe.MUTATION_FLOOR / 10
    assert e_gpu <= C * e_ref32
    assert lq.shape == h["lq64"].shape and l_gpu <= 2 * l_ref32
    assert torch.equal(preds.long(), tim_probe.first_argmax(lq))


# ---- the in-place entries: the probed weights have the bits of the dense call -------------------------------------------------

def _tables(x, cols, gen):
    """(table, idx): the rows of x (T,R,D) at shuffled positions of a table twice as long (noise elsewhere), stored so that
    table[idx[t]][:, cols[t]] == x[t] (cols None: table[idx] == x)"""
    T, R, D = x.shape
    pos = torch.randperm(2 * T * R + 3, generator=gen)[:T * R].view(T, R)
    table = torch.randn(2 * T * R + 3, D, generator=gen)
    if cols is not None:
        stored = torch.empty_like(x)
        stored.scatter_(2, cols.long().unsqueeze(1).expand(T, R, D), x)                # stored[t, r, cols[t, d]] = x[t, r, d]
        x = stored
    table[pos.reshape(-1)] = x.reshape(T * R, D)
    return table, pos


# K >= 960 with the flip permutation and an odd Q; a full first register slot with a random permutation; interior tiles on the
# 128-bit path with a partial last slice of R, no permutation (visual features take none)
IN_PLACE = [((None, True, 1023, 1023, 1, 75, 1, 15.0), "flip"), (("AAA7", True, 64, 64, 1, 77, 3, 5.0), "random"),
            (("SAA2", False, 96, 128, 1, 77, 3, 5.0), None)]


def test_in_place_cases_are_cases_of_the_sweep():
    assert all(c in CASES for c, _ in IN_PLACE)
    assert any(c[3] >= 960 and p == "flip" for c, p in IN_PLACE) and any(c[5] % 2 for c, _ in IN_PLACE)
    assert {c[0] is None for c, _ in IN_PLACE} == {True, False}


@pytest.mark.parametrize("case,perm", IN_PLACE, ids=lambda v: case_id(v) if isinstance(v, tuple) else str(v))
def test_in_place_probed_weights_have_the_dense_bits(case, perm):
    h = host_side(case)
    _, _, D, K, _, _, T, _ = case
    gen = torch.Generator().manual_seed(D * 31 + K)
    cols = None
    if perm == "flip":
        cols = torch.arange(D - 1, -1, -1, dtype=torch.int32).repeat(T, 1)
    elif perm == "random":
        cols = torch.stack([torch.randperm(D, generator=gen) for _ in range(T)]).to(torch.int32)
    table_s, s_idx = _tables(h["x_s"], cols, gen)
    table_q, q_idx = _tables(h["x_q"], cols, gen)
    table_s, table_q = table_s.to(DEV), table_q.to(DEV)
    x_q, x_s, y_s = h["x_q"].to(DEV), h["x_s"].to(DEV), h["y_s"].to(DEV)
    take = None if cols is None else cols.long().to(DEV).unsqueeze(1)
    for table, idx, x in ((table_s, s_idx, x_s), (table_q, q_idx, x_q)):               # the tables do hold the dense rows
        rows = table[idx.to(DEV)]
        assert torch.equal(rows if take is None else torch.gather(rows, 2, take.expand_as(rows)), x)
    dense, kw = engine_entry(case)
    tasks, _ = engine_entry(case, tasks=True)
    extra = () if not case[1] and case[0] is not None else (cols,)                     # run_alpha_tim_visual_tasks takes no cols
    s = tim_probe.scales(h["g64"])
    for j in range(tim_probe.N_SCALES):
        lw = [w * s[j] for w in h["prm"]["loss_weights"]]
        want = dense(x_q, x_s, y_s, loss_weights=lw, **kw)
        got = tasks(table_q, q_idx, table_s, s_idx, h["y_s"], *extra, loss_weights=lw, **kw)
        for name, a, b in zip(("weights", "logits_q", "preds", "criterions"), got, want):
            a, b = a.cpu().contiguous(), b.cpu().contiguous()
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (name, j)
        if j == 0:                                                                     # the largest element is read at this scale
            moved = (h["w0"] - want[0].cpu().double()).abs()
            assert bool(((moved >= tim_probe.A_LO) & (moved <= tim_probe.A_HI)).any())
