"""The four operand pack passes of the packed GEMM, restated in numpy from the
layout comments of csrc/gemm_x3p.h and csrc/x3p_common.h.  Their output is a
pure function of the input, so the kernels are compared with it bit for bit.

Split-fp16 (x3p): a packed row is scaled by 2^e, e = 14 - frexp(max |row|)[1]
(14 for an all-zero row; from the bound when one is given), which puts the
row's maximum in [2^13, 2^14).  Each scaled value x = ldexp(float32 v, e) is
split into hi = float16(x) and lo = float16(x - float32(hi)).  Layout
[rows][KB][64] halves: per block of 32 k, 32 hi then 32 lo halves, zero past
the last k.

bf16: round to nearest even on the upper 16 bits, [rows][KB][64] over blocks
of 64 k, zero past the last k.

Column kinds pack the transpose: packed row c is column c of X [R][Cn], with
out[c][k] = X[k - shift][c] where 0 <= k < R and 0 <= k - shift < R, else 0."""
import numpy as np


def split_exp(mx):
    """Exponent of a row whose max |x| (or bound) is mx (float32 array or scalar)."""
    return (14 - np.frexp(np.asarray(mx, dtype=np.float32))[1]).astype(np.int32)


def bf16_bits(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def pad_k(rows, block):
    """rows [n][K] -> [n][KB][block], zero past K."""
    n, K = rows.shape
    KB = (K + block - 1) // block
    out = np.zeros((n, KB * block), np.float32)
    out[:, :K] = rows
    return out.reshape(n, KB, block)


def transpose_shifted(X, shift):
    """T [Cn][R]: T[c][k] = X[k - shift][c], zero where k - shift is outside [0, R)."""
    R, Cn = X.shape
    T = np.zeros((Cn, R), np.float32)
    for k in range(R):
        if 0 <= k - shift < R:
            T[:, k] = X[k - shift, :]
    return T


def x3p_split(rows, e):
    """rows [n][K] float32, e [n] int32 -> uint16 [n][KB][64]."""
    x = pad_k(rows, 32)
    x = np.ldexp(x, e[:, None, None].astype(np.int32)).astype(np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return np.concatenate([hi, lo], axis=2).view(np.uint16)


def x3p_rows(X, bound=0.0):
    """-> (uint16 [R][KB][64], int32 [R])"""
    X = np.asarray(X, dtype=np.float32)
    mx = np.abs(X).max(axis=1)
    e = split_exp(np.full_like(mx, bound) if bound > 0 else mx)
    return x3p_split(X, e), e


def x3p_cols(X, shift=0, cmax=None, bound=0.0):
    """X [R][Cn]; cmax: float32 max |x| per column (unused with a bound) ->
    (uint16 [Cn][KB][64], int32 [Cn])"""
    X = np.asarray(X, dtype=np.float32)
    e = split_exp(np.full(X.shape[1], bound, np.float32) if bound > 0 else cmax)
    return x3p_split(transpose_shifted(X, shift), e), e


def bf16_rows(X):
    return bf16_bits(pad_k(np.asarray(X, dtype=np.float32), 64))


def bf16_cols(X, shift=0):
    return bf16_bits(pad_k(transpose_shifted(np.asarray(X, dtype=np.float32), shift), 64))


def x3p_unpack(packed, e):
    """The values a packed operand stands for: 2^-e (hi + lo), float64 [n][KB * 32]."""
    h = packed.view(np.float16).astype(np.float64)
    v = h[:, :, :32] + h[:, :, 32:]
    return np.ldexp(v, -e[:, None, None].astype(np.int32)).reshape(packed.shape[0], -1)
