"""The reference host's float32 logarithm and batched matrix product on every host.

torch.log on the host is MKL's vsLn, whose kernel follows the host's CPU: on the machine the fixtures were made on it is the one
csrc/tclip_math.h restates (log_f32; tests/test_math_host.py pins the two to each other there), on another CPU vendor it is a few
ulp off on a fraction of the arguments.  restated_log() is that restatement's host build (oracle/mathcheck.cpp, mc_log): the same
bits on every host.  The torch restatements of oracle/ref_torch.py and tests/helpers/visual_cov.py take it as their `log`.

torch.bmm on the host is MKL's sgemm, which picks its kernel by the host's CPU as well.  On the fixture host every output of
KL_KMEANS's u^T z is one chain of fused multiply-adds over the query rows in ascending order (k_kl_centroids restates that;
scripts/host_bmm_check.py probes it against the host's torch); a host was met where rows of 7 elements, 15 or more of them,
are summed in another order.  restated_bmm() is the chain's host build (oracle/mathcheck.cpp, mc_bmm_tn), and
ref_torch.run_kl_kmeans takes it as its `bmm`; tests/test_restated_log_fixtures.py pins it to the reference-made fixtures."""
import ctypes

import numpy as np
import torch


def _mathcheck():
    from oracle import build as oracle_build
    return ctypes.CDLL(oracle_build.build()[1])


def restated_log():
    """x -> log(x) for a float32 tensor, MKL's vsLn as the reference's host evaluates it"""
    lib = _mathcheck()

    def log(x):
        assert x.dtype == torch.float32, "the restated logarithm is the float32 one"
        a = np.ascontiguousarray(x.numpy(), np.float32)
        y = np.empty_like(a)
        lib.mc_log(a.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(a.size))
        return torch.from_numpy(y)
    return log


def restated_bmm():
    """(a (T,M,R), b (T,R,N)) -> a @ b (T,M,N) for float32 tensors, as the reference's host evaluates KL_KMEANS's u^T z"""
    lib = _mathcheck()

    def bmm(a, b):
        assert a.dtype == b.dtype == torch.float32 and a.dim() == b.dim() == 3 and a.shape[0] == b.shape[0] and a.shape[2] == b.shape[1]
        T, M, R = a.shape
        N = b.shape[2]
        at = np.ascontiguousarray(a.transpose(1, 2).numpy(), np.float32)          # (T, R, M): both operands by rows of the sum
        bt = np.ascontiguousarray(b.numpy(), np.float32)
        out = np.empty((T, M, N), np.float32)
        ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        lib.mc_bmm_tn(ptr(at), ptr(bt), ctypes.c_long(T), ctypes.c_long(R), ctypes.c_long(M), ctypes.c_long(N), ptr(out))
        return torch.from_numpy(out)
    return bmm
