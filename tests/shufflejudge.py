"""Shared by tests/test_shuffle_train_cpu.py and tests/test_gpu_shuffle_train.py: the numpy oracle of the padded weight images of
ssdk_pws_prepare and the operands of the ShuffleNetV2 training kernels (drawn as tests/dwjudge.py draws them: N(0, 1) in the dtype,
weights as fp32 masters holding rounded values)."""
import numpy as np
import torch

PREPARE_SHAPES = [(58, 24), (58, 58), (122, 244)]  # (Cout, Cin)


def pad8(v):
    return (int(v) + 7) // 8 * 8


def prepare_oracle(w):
    """w [Cout, Cin] (numpy, values already representable in the 16-bit dtype) -> (w16 [Cout, Kp], wt16 [Cin, Mp]) as float32 arrays:
    row-major, rows zero-padded to Kp = 8 ceil(Cin / 8) and Mp = 8 ceil(Cout / 8) columns (include/ssdk_shuffletrain.h)."""
    cout, cin = w.shape
    w16 = np.zeros((cout, pad8(cin)), dtype=np.float32)
    wt16 = np.zeros((cin, pad8(cout)), dtype=np.float32)
    w16[:, :cin] = w
    wt16[:, :cout] = w.T
    return w16, wt16


def weights(cout, cin, dtype, seed):
    """fp32 master weights [Cout, Cin, 1, 1] holding values of ``dtype``."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).to(dtype).float()


def tensor(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)
