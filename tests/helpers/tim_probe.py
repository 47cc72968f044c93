"""Reading the gradient of ALPHA_TIM / TIM_GD out of one Adam step, through nothing but a method's public entry.

One step from zero state with iters = 1, lr = 1 moves every weight by  w0 - w1 = g / (|g| + 1e-8)  (m = 0.1 g, v = 0.001 g^2, the
bias corrections cancel; k_tim_adam and torch.optim.Adam alike).  g is linear in the three loss weights, so a run with
`loss_weights * s`, s chosen so that s |g| is near 1e-8, leaves  a = |w0 - w1|  away from 0 and 1, and then

    g = 1e-8 (w0 - w1) / ((1 - a) s).

`probe` walks a ladder of 15 scales half a decade apart (seven decades of |g|) and reads every element at the scale where a is
nearest 0.5, if that a lies in [0.2, 0.8] (a span of 16 in s |g|, against the ladder's step of 3.16).  It takes a callable
run(loss_weights) -> weights, so an engine entry and a torch restatement go through the same code.  w0 (the class means of the
support rows) and g64 come from the restatement's loss_gradient in float64.

ENTROPIES: the four ALPHA_TIM combinations the gradient tests use, with weights, alpha and temperature at which every one of the
three terms carries weight in the gradient (tests/test_tim_gradient_probe.py asserts that on the restatement)."""
import numpy as np
import torch

ADAM_EPS = 1e-8
N_SCALES = 15
A_LO, A_HI = 0.2, 0.8

# The ALPHA_TIM settings of the gradient tests.  AAA7: at alpha = 7 the marginal term 7 m^6 / 6 is orders below the conditional
# one at equal weights, hence loss_weights[1] = 100; and the reference's Alpha cross-entropy, pow(hot, a) * pow(p + 1e-12, 1 - a),
# is 0 * inf in fp32 once a class probability of a support row falls below 10^-6.4, hence temp = 5 (p >= exp(-5) / K there)
ENTROPIES = {
    "SSS": dict(entropies=("Shannon", "Shannon", "Shannon"), alpha_value=2.0, loss_weights=(1.0, 0.7, 1.2), temp=15.0),
    "SAA2": dict(entropies=("Shannon", "Alpha", "Alpha"), alpha_value=2.0, loss_weights=(1.0, 0.7, 1.2), temp=15.0),
    "AAA7": dict(entropies=("Alpha", "Alpha", "Alpha"), alpha_value=7.0, loss_weights=(1.0, 100.0, 3.0), temp=5.0),
    "ASS05": dict(entropies=("Alpha", "Shannon", "Shannon"), alpha_value=0.5, loss_weights=(1.0, 0.7, 1.2), temp=15.0),
}
GD = dict(loss_weights=(1.0, 0.7, 1.2), temp=15.0)
# the smallest e that a 1 % change of one loss weight gives on the restatement (tests/test_tim_gradient_probe.py asserts it)
MUTATION_FLOOR = 8e-2


def scales(g64):
    """s_j = 1e-8 / max|g64| * 10^(j/2), j = 0..14"""
    top = float(g64.abs().max())
    assert top > 0
    return [ADAM_EPS / top * 10.0 ** (j / 2) for j in range(N_SCALES)]


def probe(run, loss_weights, w0, g64):
    """run(loss_weights) -> weights (T,K,D) after ONE Adam step at lr = 1 (any float dtype, any device).
    -> (g (T,K,D) float64, measured (T,K,D) bool): the gradient at `loss_weights` as read from the steps; g is 0 where no
    scale gave an a in [0.2, 0.8]"""
    best_a = torch.full(w0.shape, float("inf"), dtype=torch.float64)
    g = torch.zeros(w0.shape, dtype=torch.float64)
    for s in scales(g64):
        w1 = run([float(w) * s for w in loss_weights]).detach().cpu().double()
        assert w1.shape == w0.shape, (w1.shape, w0.shape)
        d = w0 - w1
        a = d.abs()
        take = (a >= A_LO) & (a <= A_HI) & ((a - 0.5).abs() < (best_a - 0.5).abs())
        g = torch.where(take, ADAM_EPS * d / ((1 - a) * s), g)
        best_a = torch.where(take, a, best_a)
    return g, torch.isfinite(best_a)


def error(x, g64, measured=None):
    """e(x) = max over the measured elements of |x - g64| / max(|g64|, 1e-3 max|g64| of that task)"""
    floor = 1e-3 * g64.abs().amax(dim=(1, 2), keepdim=True)
    rel = (x.double() - g64).abs() / torch.maximum(g64.abs(), floor)
    if measured is not None:
        rel = torch.where(measured, rel, torch.zeros_like(rel))
    return float(rel.max())


def share_left_out(measured):
    return 1.0 - float(measured.double().mean())


def first_argmax(logits):
    """the first maximum of every row (numpy's argmax), as k_tim_softmax picks it"""
    return torch.from_numpy(np.argmax(logits.cpu().numpy(), axis=-1))


def make_inputs(prob, D, K, shots, Q, T):
    """-> (x_q (T,Q,D), x_s (T,K*shots,D), y_s (T,K*shots)), CPU tensors seeded by the shape.  prob: peaked probability rows
    (D = K; tclip_amd.synth, queries from four classes); otherwise normal rows of norm about 1 in a seeded label order"""
    seed = ((D * 1031 + K) * 131 + Q) * 7 + shots
    if prob:
        from tclip_amd import synth
        assert D == K
        x_q, _ = synth.make_query_tasks(T, K, seed=seed, n_query=Q, k_eff=min(4, K))
        x_s, y_s = synth.make_support(T, K, shots, seed=seed)
        return x_q, x_s, y_s.squeeze(2).contiguous()
    from helpers import visual_fs
    x_s, y_s, x_q = visual_fs.random_tasks(T, K, D, shots, seed, n_query=Q, scale=1.0 / D ** 0.5)
    return x_q, x_s, y_s


def restatement(ent, x_q, x_s, y_s, K, temp=None):
    """ent: None (TIM_GD) or a key of ENTROPIES; temp: in place of the setting's own -> (prm: the method's parameters, loss
    weights among them; grad(dtype, loss_weights) -> (w0, gradient, logits_q) by autograd; run(loss_weights) -> the fp32
    restatement's weights after one Adam step at lr = 1)"""
    from helpers import alpha_tim, tim_gd
    mod, prm = (tim_gd, dict(GD)) if ent is None else (alpha_tim, dict(ENTROPIES[ent]))
    if temp is not None:
        prm["temp"] = float(temp)
    rest = {k: v for k, v in prm.items() if k != "loss_weights"}
    run_loop = tim_gd.run_tim_gd if ent is None else alpha_tim.run_alpha_tim

    def grad(dtype, loss_weights):
        return mod.loss_gradient(x_q, x_s, y_s, n_class=K, loss_weights=loss_weights, dtype=dtype, **rest)

    def run(loss_weights):
        return run_loop(x_q, x_s, y_s, n_class=K, iters=1, lr=1.0, loss_weights=loss_weights, **rest)["weights"]
    return prm, grad, run


def term_gradients(grad):
    """the float64 gradient of each of the three loss terms alone (loss weights (1,0,0), (0,1,0), (0,0,1)): the gradient is
    linear in the weights, so g64 at any weights is their combination, and so is g64 with one weight times 1.01"""
    return [grad(torch.float64, [1.0 if j == i else 0.0 for j in range(3)])[1] for i in range(3)]


def balanced_weights(terms):
    """loss weights (1, b, c), two significant digits, at which the three terms' largest gradient elements are equal: no term
    drowns in another.  (At alpha = 7 the Alpha cross-entropy's p^-7 is 5 to 16 orders above the entropy terms' p^6.)"""
    tops = [float(t.abs().max()) for t in terms]
    assert all(0 < t < float("inf") for t in tops), tops
    return [1.0] + [float(f"{tops[0] / t:.2g}") for t in tops[1:]]


def mutation_errors(terms, loss_weights):
    """-> (g64 at `loss_weights`, [e(g64 with loss weight i times 1.01) for i = 0, 1, 2]): what a 1 % change of each term alone
    does to the metric on these inputs"""
    g64 = sum(w * t for w, t in zip(loss_weights, terms))
    return g64, [error(g64 + 0.01 * w * t, g64) for w, t in zip(loss_weights, terms)]
