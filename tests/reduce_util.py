"""The order-free fixed-point M-step of gdd.sharded.ShardedKMeans(mstep="reduce") restated in numpy
(include/gdd.h states the arithmetic): the CPU stand-in of the three device phases, test-only."""
import numpy as np
import torch

from sharded_util import OracleOps, _np


def reduce_exponents(Xc):
    """e_f = 62 - bit_length(n - 1) - frexp_exponent(max_i |Xc[i, f]|), 0 for an all-zero column."""
    amax = np.abs(Xc).max(axis=0)
    L = int(Xc.shape[0] - 1).bit_length()
    return np.where(amax > 0, 62 - L - np.frexp(amax)[1], 0).astype(np.int32)


def reduce_local(Xc, labels, labels_old, k, exps, r0, r1):
    """The int64 buffer of rows [r0, r1): k*dim sums of q, k counts, the changed count (labels_old is
    updated on those rows)."""
    dim = Xc.shape[1]
    lab = labels[r0:r1]
    q = np.rint(np.ldexp(Xc[r0:r1].astype(np.float64), exps)).astype(np.int64)
    buf = np.zeros(k * dim + k + 1, np.int64)
    np.add.at(buf[:k * dim].reshape(k, dim), lab, q)
    buf[k * dim:k * dim + k] = np.bincount(lab, minlength=k)
    buf[-1] = np.count_nonzero(lab != labels_old[r0:r1])
    labels_old[r0:r1] = lab
    return buf


def reduce_sums32(buf, k, dim, exps):
    """(fp32 sums, fp32 weights) of a reduced buffer: one int64 -> fp32 rounding, an exact scaling."""
    sums = np.ldexp(buf[:k * dim].reshape(k, dim).astype(np.float32), -exps).astype(np.float32)
    return sums, buf[k * dim:k * dim + k].astype(np.float32)


class ReduceOps(OracleOps):
    def lloyd_reduce_begin(self, ctx):
        ctx.rbuf = torch.zeros(ctx.k * ctx.dim + ctx.k + 1, dtype=torch.int64)
        ctx.exps = np.zeros(ctx.dim, np.int32)

    def lloyd_reduce_exponents(self, ctx, X):
        ctx.exps[:] = reduce_exponents(_np(X))

    def lloyd_reduce_local(self, ctx, X, r0, r1, it):
        ctx.rbuf.zero_()  # not gated, as on the device
        if self._stopped(ctx, 2 * it):
            return
        ctx.rbuf.copy_(torch.from_numpy(reduce_local(_np(X), ctx.labels[:ctx.n].numpy(),
                                                     ctx.labels_old.numpy(), ctx.k, ctx.exps, r0, r1)))

    def lloyd_reduce_update(self, ctx, from_cnew, C_new, C_old, tol, it):
        if self._stopped(ctx, 2 * it + 1):
            return
        k, dim = ctx.k, ctx.dim
        if not from_cnew:
            buf = ctx.rbuf.numpy()
            sums, w = reduce_sums32(buf, k, dim, ctx.exps)
            C_new.copy_(torch.from_numpy(sums))
            ctx.wsum.copy_(torch.from_numpy(w))
            if buf[-1] != 0:
                ctx.state.changed = 1
            if np.any(buf[k * dim:k * dim + k] == 0):
                ctx.state.reason, ctx.state.iter, ctx.state.stop_at = 3, it, 2 * it + 1
                return
        cn, shift = self.average(C_new, ctx.wsum, C_old)
        C_new.copy_(cn)
        ctx.shift.copy_(shift)
        reason = 0
        if ctx.state.changed == 0:
            reason = 1
        elif float((shift.numpy() ** 2).sum()) <= tol:  # numpy's pairwise fp32 sum
            reason = 2
        ctx.state.changed = 0
        ctx.state.done = it + 1
        if reason:
            ctx.state.reason, ctx.state.iter, ctx.state.stop_at = reason, it, 2 * it + 2
