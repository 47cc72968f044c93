"""GPU: both instantiations of k_probability_features - features.probability_features (tclip_probability_features: the scale
before the product, softmax(T * normalize(f) @ text.T), src/utils.py:287-290) and engine.visual_init (tclip_visual_init: the
scale after it, soft_kmeans.py:185-197) - against float64 and fp32 torch restatements of the same formula
(tests/helpers/accuracy_tail.py), over D = 1 .. 1024 (the 16-byte loads need D % 4 == 0; blocks of 64 products), K = 1 .. 1024
(a block has 256 threads), one row and 65 rows, T = 10, 30, 100, on random rows (3 * randn) and structured ones
(2 * text[label] + noise).  The reference ran this through cuBLAS: there are no reference bits, hence bounds.

  relative error   e(gpu) <= 3 e(ref32), e(a) = max |a - ref64| / ref64 over ALL probabilities, ref32 torch's fp32 formula of
                   the same scale order.  Every ref64 probability is >= 1e-32 (asserted), so every fp32 one is normal and none
                   is left out.  The factor is the one of tests/test_gpu_tim_gradient.py, for its reason: block sums of 64
                   products against torch's GEMM order - two orders, so the ratio is not 1.
  told apart       on sparse rows at T = 100 (accuracy_tail.SWAP_CASES: there the scale order is what is left of the rounding)
                   each entry is closer to its own fp32 formula than to the other's.
  properties       rows sum to 1 within 1e-5; the argmax is ref64's wherever ref64's two largest differ by more than 1e-5
                   relative; K = 1 gives exactly 1.0.
  rejected calls   dim + n_class > 15000 is TCLIP_ERR_ARG from both entries with nothing written; n_rows = 0 is TCLIP_OK.
  alignment        text given as a view one float into a larger buffer (16-byte loads are not possible) gives the bits of
                   the aligned call.

Largest e(gpu) / e(ref32) per D, measured on an MI355X: DESIGN.md 8k."""
import ctypes

import pytest
import torch

from helpers import accuracy_tail as at

pytestmark = pytest.mark.gpu
C = 3.0
ENTRIES = [False, True]                    # scale_after
entry_id = {False: "probability_features", True: "visual_init"}.get


def check_case(shape, kind):
    c = at.front_case(shape, kind)         # asserts min ref64 >= 1e-32
    failed = []
    for after in ENTRIES:
        z = at.run_front_end(c["f"], c["text"], c["T"], after)
        ref64, ref32 = c["ref64", after], c["ref32", after]
        assert z.shape == ref64.shape and z.dtype == torch.float32
        e_gpu, e_ref = at.rel_err(z, ref64), at.rel_err(ref32, ref64)
        print(f"{at.front_id(shape)} {kind} {entry_id(after)}: e(gpu) {e_gpu:.3e}  e(ref32) {e_ref:.3e}  "
              f"ratio {e_gpu / e_ref if e_ref else float(e_gpu > 0):.3f}  min ref64 {float(ref64.min()):.1e}")
        if not e_gpu <= C * e_ref:
            failed.append(f"{entry_id(after)}: e(gpu) {e_gpu:.3e} > {C:g} x e(ref32) {e_ref:.3e}")
        if not float((z.sum(-1) - 1).abs().max()) <= 1e-5:
            failed.append(f"{entry_id(after)}: a row sums to 1 + {float((z.sum(-1) - 1).abs().max()):.2e}")
        if shape[2] == 1:
            if not bool((z == 1.0).all()):
                failed.append(f"{entry_id(after)}: K = 1 must give exactly 1.0")
        else:
            top = ref64.topk(2, dim=-1).values
            clear = (top[:, 0] - top[:, 1]) > 1e-5 * top[:, 0]
            if not torch.equal(z.argmax(-1)[clear], ref64.argmax(-1)[clear]):
                failed.append(f"{entry_id(after)}: argmax differs from ref64's on a row whose two largest are apart")
    return failed


@pytest.mark.parametrize("kind", at.FRONT_KINDS)
@pytest.mark.parametrize("shape", at.FRONT_SHAPES, ids=at.front_id)
def test_front_end_within_three_times_torchs_fp32_error(shape, kind):
    failed = check_case(shape, kind)
    assert not failed, (at.front_id(shape), kind, failed)


@pytest.mark.parametrize("shape", at.SWAP_CASES, ids=at.front_id)
def test_the_two_scale_orders_are_told_apart(shape):
    c = at.front_case(shape, "sparse")
    assert int((c["ref32", False] != c["ref32", True]).sum()) > 0
    for after in ENTRIES:
        z = at.run_front_end(c["f"], c["text"], c["T"], after)
        own = at.front_distance(z, c["ref32", after], c["ref64", after])
        other = at.front_distance(z, c["ref32", not after], c["ref64", after])
        print(f"{at.front_id(shape)} {entry_id(after)}: rms distance to its own fp32 formula {own:.3e}, to the other's {other:.3e}")
        assert own < other, entry_id(after)


def _raw(name, f, text, n_rows, D, K, out, T=30.0):
    from tclip_amd import _capi
    fn = getattr(_capi.lib(), name)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = fn(P(f), P(text), ctypes.c_int64(n_rows), ctypes.c_int32(D), ctypes.c_int32(K), ctypes.c_float(T), P(out),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", ["tclip_probability_features", "tclip_visual_init"])
def test_rejected_and_empty_calls(name):
    """the sizes are checked before anything is launched, so the small buffers here are never indexed"""
    f, text = torch.ones(4, 8, device="cuda"), torch.ones(4, 8, device="cuda")
    out = torch.full((4, 4), -7.0, device="cuda")
    for D, K in ((14000, 1001), (1, 15000), (15000, 1)):
        assert D + K > 15000
        assert _raw(name, f, text, 1, D, K, out) == 1, (D, K)                  # TCLIP_ERR_ARG
    assert _raw(name, f, text, 0, 8, 4, out) == 0                                # TCLIP_OK, nothing to do
    assert bool((out == -7.0).all())
    assert _raw(name, f, text, 4, 8, 4, out) == 0
    assert float((out - 0.25).abs().max()) < 1e-6                                # equal logits: uniform rows


@pytest.mark.parametrize("after", ENTRIES, ids=entry_id)
@pytest.mark.parametrize("shape", [(65, 512, 100, 100), (5, 64, 37, 30), (3, 4, 2, 30)], ids=at.front_id)
def test_text_at_a_four_byte_offset_gives_the_aligned_bits(shape, after):
    """a contiguous view that starts one float into its buffer stays as it is under .contiguous(): its rows are not 16-byte
    aligned and the entries have to take the scalar loop for them"""
    c = at.front_case(shape, "random")
    n, D, K, _ = shape
    aligned = at.run_front_end(c["f"], c["text"], c["T"], after)
    buf = torch.zeros(K * D + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + K * D].view(K, D)
    view.copy_(c["text"])
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    from tclip_amd import engine, features
    got = (engine.visual_init if after else features.probability_features)(c["f"].cuda(), view, c["T"])
    torch.cuda.synchronize()
    assert torch.equal(got.cpu().view(torch.int32), aligned.view(torch.int32))
