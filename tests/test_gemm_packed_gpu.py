"""The packed GEMM (gemm_x3p / gemm_x3p_pair) on its own, through the
kcm_test_gemm_packed hook: fp32 operands A [M][K], B [N][K] are packed
(x3p_pack_rows or bf16_pack_rows) and multiplied into C [M][N] = A B^T.

Each case is the smallest shape on which its path can still go wrong: ragged
128- and 256-tile shapes, split-K with an uneven last chunk (K = 1024 in three
chunks: 11 / 11 / 10 k blocks of 32 for split-fp16, 6 / 6 / 4 of 64 for bf16),
the pair launch, and a persistent grid smaller than its tile count with and
without a tile counter.

Split-fp16: against the float64 product under test_gemm_x3_matches_numpy's
bars.  bf16: against the float64 product of the operands rounded to bf16
(round to nearest even on the upper 16 bits); bf16 x bf16 products are exact
in fp32, so only the K - 1 additions round, (K - 1) 2^-24 (|A| |B|)_ij in all;
the bar is K 2^-23 (|A| |B|)_ij, twice that, to cover the matrix core's
internal accumulation order."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

# (id, M, N, K, split, dynamic, max_blocks, M2)
CASES = [
    ("t128_ragged", 130, 70, 96, 1, 0, 0, 0),
    ("t256_ragged", 300, 260, 257, 1, 0, 0, 0),
    ("t128_split3", 130, 70, 1024, 3, 0, 0, 0),
    ("t256_split3", 300, 260, 1024, 3, 0, 0, 0),
    ("pair", 300, 260, 257, 1, 1, 0, 200),
    ("persistent", 1300, 800, 64, 1, 0, 8, 0),
    ("persistent_dynamic", 1300, 800, 64, 1, 1, 8, 0),
]


def bf16_round(x):
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def check(name, out, A, B, K, bf16):
    assert np.all(np.isfinite(out)), name
    out = out.astype(np.float64)
    if bf16:
        a, b = bf16_round(A).astype(np.float64), bf16_round(B).astype(np.float64)
        ref = a @ b.T
        bar = K * 2.0 ** -23 * (np.abs(a) @ np.abs(b).T)
        worst = np.max(np.abs(out - ref) / bar)
        print(f"{name} bf16: max |C - ref| / bar = {worst:.2e}")
        assert worst <= 1.0
    else:
        ref = A.astype(np.float64) @ B.T.astype(np.float64)
        scale = np.abs(A).max(axis=1)[:, None] * np.abs(B).max(axis=1)[None, :] * K
        worst, rel = np.max(np.abs(out - ref) / scale), rel_err(out, ref)
        print(f"{name} fp16: max |C - ref| / scale = {worst:.3e}, rel_err = {rel:.3e}")
        assert worst < 2e-7
        assert rel < 1e-6


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gemm_packed(kctc, gpu, case, bf16):
    import torch
    name, M, N, K, split, dynamic, max_blocks, M2 = case
    rng = np.random.default_rng(M * 7 + N + K + split)
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((N, K)).astype(np.float32)
    if not bf16:  # rows spanning 1e-12 .. 1e6: the per-row exponents matter
        A *= (10.0 ** rng.uniform(-12, 6, M)).astype(np.float32)[:, None]
        B *= (10.0 ** rng.uniform(-12, 6, N)).astype(np.float32)[:, None]
    dA, dB = torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu)
    dC = torch.full((M, N), float("nan"), dtype=torch.float32, device=gpu)
    dC2 = torch.full((M2, N), float("nan"), dtype=torch.float32, device=gpu) if M2 else None
    rc = kctc.lib().kcm_test_gemm_packed(None, M, N, K, bf16, split, dynamic, max_blocks, M2, dA.data_ptr(),
                                         dB.data_ptr(), dC.data_ptr(), dC2.data_ptr() if M2 else None)
    assert rc == 0
    torch.cuda.synchronize()
    check(name, dC.cpu().numpy(), A, B, K, bf16)
    if M2:
        check(name + " C2", dC2.cpu().numpy(), A[:M2], B, K, bf16)
