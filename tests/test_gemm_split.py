"""gemm_pick_split (csrc/gemm.hip), the split-K heuristic of the fp32 GEMM:
what its callers rely on when they size the split-K workspace from it.  Host
code only; no GPU."""
import itertools


def test_gemm_pick_split_contract(kctc):
    L = kctc.lib()
    dims, ks = [1, 41, 128, 129, 2048], [0, 127, 128, 1000, 32000]
    for M, N, K, batch in itertools.product(dims, dims, ks, [1, 2]):
        s = L.kcm_test_gemm_pick_split(M, N, K, batch)
        assert 1 <= s <= 64, (M, N, K, batch, s)
        if K < 128:
            assert s == 1, (M, N, K, batch, s)
        # gemm_f32 cuts K into chunks of ceil(K / s) rounded up to the k tile of
        # 32 and runs one slab per chunk: never more than the s the workspace
        # was sized for, and no slab is empty
        used = L.kcm_test_gemm_split_used(K, s)
        if s > 1:
            kchunk = (-(-K // s) + 31) // 32 * 32
            assert used == -(-K // kchunk), (M, N, K, batch, s, used)
            assert (used - 1) * kchunk < K
        assert 1 <= used <= s, (M, N, K, batch, s, used)


def test_gemm_split_used_edges(kctc):
    L = kctc.lib()
    # (K, split asked) -> slabs run: the table of test_gemm_f32_gpu.test_split_k, K = 0 and no split
    for K, s, used in [(200, 3, 3), (130, 5, 5), (65, 4, 3), (20, 2, 1), (0, 3, 1), (1000, 1, 1), (4096, 64, 64)]:
        assert L.kcm_test_gemm_split_used(K, s) == used, (K, s)
