"""numpy restatement of gingr_amd/csrc/gpmm_plan.h, the host-side bookkeeping of the GPMM construction: column count of the generic
factorisation from the scalar traces, eigen blocks, merge of the coordinate spectra, and what gingr_gpmm_info reports.  The same
floating-point operations in the same order (IEEE double, no fused multiply-add)."""
import numpy as np

NONE, CEILING_BEFORE_TOLERANCE, ABOVE_RANK_LIMIT = 0, 1, 2


def generic_trace(htr, n):
    """residual trace after n = 3j + e generic pivots: (3 - e) tr_s(j) + e tr_s(j + 1)"""
    j, e = divmod(n, 3)
    return 3.0 * float(htr[j]) if e == 0 else float(3 - e) * float(htr[j]) + float(e) * float(htr[j + 1])


def count_columns(htr, ks, limit, rel_tol, M):
    tr0 = 3.0 * float(htr[0])
    tol = rel_tol * tr0
    n = 0
    while n < min(limit, 3 * ks) and generic_trace(htr, n) >= tol:          # a NaN trace compares false and stops
        n += 1
    tr = generic_trace(htr, n)
    cnt = [n // 3 + (1 if d < n % 3 else 0) for d in range(3)]
    with np.errstate(all="ignore"):
        fraction = float(np.float64(tr) / np.float64(tr0))
    return n, cnt, (not tr >= tol) or n == 3 * M, fraction


def group(keys, skip=lambda k: False):
    """group_of[d] (-1 where skipped) and the key of every group, in order of first appearance"""
    firsts, group_of = [], []
    for k in keys:
        if skip(k):
            group_of.append(-1)
            continue
        if k not in firsts:
            firsts.append(k)
        group_of.append(firsts.index(k))
    return group_of, firsts


def group_blocks(cnt):
    block_of, block_n = group(cnt, lambda c: c == 0)
    return len(block_n), block_of, block_n + [0] * (3 - len(block_n))


def merge_spectra(ev, cnt, block_of):
    """columns by eigenvalue descending, then index within the block, then coordinate"""
    lam = np.array([ev[block_of[d]][i] for d in range(3) for i in range(cnt[d])], dtype=np.float64)
    dim = np.array([d for d in range(3) for i in range(cnt[d])], dtype=np.int64)
    idx = np.array([i for d in range(3) for i in range(cnt[d])], dtype=np.int64)
    order = np.lexsort((dim, idx, -lam))
    lam, dim, idx = lam[order], dim[order], idx[order]
    return np.where(lam > 0.0, lam, 0.0), dim, np.array(block_of, dtype=np.int64)[dim], idx


def eigvecs_needed(qblock, qidx, keep):
    return [int(max([i + 1 for b_, i in zip(qblock[:keep], qidx[:keep]) if b_ == b], default=0)) for b in range(3)]


def conclude(ex, to_tolerance, keep_rank, columns, reached, fraction, lam):
    """(refusal, keep, (columns, rank, tolerance_reached, residual_fraction, kept_variance_fraction))"""
    if to_tolerance and not reached:
        return CEILING_BEFORE_TOLERANCE, None, (columns, 0, 0, fraction, 1.0)
    keep = keep_rank if ex and 0 < keep_rank < columns else columns
    sums = np.cumsum(np.asarray(lam[:columns], dtype=np.float64))                  # left to right
    kept = float(sums[keep - 1] / sums[-1]) if sums[-1] > 0.0 else 1.0
    return (ABOVE_RANK_LIMIT if ex and keep > 512 else NONE), keep, (columns, keep, 1 if reached else 0, fraction, kept)
