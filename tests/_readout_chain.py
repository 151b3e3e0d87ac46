"""ndcn_readout_bwd_f32's arithmetic restated in numpy (csrc/readout_bwd.hip, include/ndcn_hip.h):
  gi[n,h]  = the sequential fp32 fma chain over c = 0 .. C-1 of gd[n,c] * Wd[c,h], from +0 (tests/_fma_chain.fma32);
  out      = a + ((((0 + p_0) + p_1) + ...) + gi), every sum rounded to fp32 on its own - the order ndcn_rk_combine_f32 has for
             lincomb(a_new, a, {p..., gi}, {1, ...}): the sum starts from +0, the base panel comes last - and gi alone when there is
             neither a base nor an addend;
  g_Wd, g_bd: the float64 sums  gd^T y  and  sum_n gd  (every fp32 x fp32 product is exact in fp64)."""
import numpy as np

from _fma_chain import fma32


def tick_gradient(gd, Wd):
    gd, Wd = np.asarray(gd, np.float32), np.asarray(Wd, np.float32)
    acc = np.zeros((gd.shape[0], Wd.shape[1]), np.float32)
    for c in range(gd.shape[1]):
        acc = fma32(gd[:, c:c + 1], Wd[c][None, :], acc)
    return acc


def combine(gi, base=None, addends=()):
    if base is None and not len(addends):
        return gi
    with np.errstate(invalid='ignore', over='ignore'):
        s = np.zeros_like(gi)
        for p in list(addends) + [gi]:
            s = (s + np.asarray(p, np.float32)).astype(np.float32)
        return s if base is None else (np.asarray(base, np.float32) + s).astype(np.float32)


def decoder_sums(gd, y):
    """(g_Wd (C, H), g_bd (C), the magnitude sums |gd|^T |y| and sum |gd|) in float64"""
    gd, y = np.asarray(gd, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    return gd.T @ y, gd.sum(0), np.abs(gd).T @ np.abs(y), np.abs(gd).sum(0)
