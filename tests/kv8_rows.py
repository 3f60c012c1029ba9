"""Edge rows of the e4m3 KV quantisation rule, shared by the CPU and GPU tests (no test in here)."""
import torch

BF16 = torch.bfloat16


def edge_rows(seed=0):
    """bf16 [8, 128]: amax exactly 448 * 2^k (k = 0, -3), just above it (the next bf16: 450), an all-zero row, rows whose
    scales lie 2^+-20 from their neighbours', and a plain one."""
    x = (torch.randn(8, 128, generator=torch.Generator().manual_seed(seed)) * 0.5).to(BF16)
    x[0, 5], x[1, 77], x[2, 0] = 448.0, -448.0 * 2.0 ** -3, 450.0
    x[3] = 0
    x[4], x[5] = x[4] * 2.0 ** 20, x[5] * 2.0 ** -20
    x[6, 127] = 3.0 * 2.0 ** -70    # (below the scale floor: the row's codes are zeros)
    x[6, :127] = 0
    return x
