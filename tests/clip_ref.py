"""The canonical reduction order of the clipped Adam step's gradient norm
(include/marlnav.h) restated in float64 numpy, operation for
operation, so that the GPU tests can ask ``norm_out`` for equal bits.

Every ``+`` below is one IEEE float64 addition of two arrays, element by
element (never ``np.sum``, whose order is numpy's own). Padding with +0.0 where
the kernels add nothing is exact: every summand is a square, so no partial sum
is -0.0."""
import numpy as np

ITEM = 4          # elements per thread
THREADS = 256     # threads per block: one block covers 1024 elements of a slot
WAVE = 64


def item_sums(g):
    """One thread: the sum of its <= 4 squares in element order, per item of
    the fp32 tensor ``g`` (a slot's last item may be short)."""
    x = np.ascontiguousarray(g, np.float32).reshape(-1).astype(np.float64)
    items = (x.size + ITEM - 1) // ITEM
    sq = np.zeros(items * ITEM, np.float64)
    sq[:x.size] = x * x
    sq = sq.reshape(items, ITEM)
    return ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]


def block_sum(v):
    """csrc/block_sum.h over rows of 256 values: per wave of 64 the shuffle
    tree as lane 0 sees it (offsets 32, 16, ..., 1), then the four waves in
    order onto 0.0."""
    w = np.array(v, np.float64).reshape(-1, THREADS // WAVE, WAVE)
    off = WAVE // 2
    while off:
        w[:, :, :off] = w[:, :, :off] + w[:, :, off:2 * off]
        off //= 2
    t = np.zeros(w.shape[0], np.float64)
    for i in range(THREADS // WAVE):
        t = t + w[:, i, 0]
    return t


def _rows(v):
    """``v`` padded with 0.0 to whole rows of 256."""
    rows = (v.size + THREADS - 1) // THREADS
    out = np.zeros(rows * THREADS, np.float64)
    out[:v.size] = v
    return out.reshape(rows, THREADS)


def block_partials(slots):
    """First stage: the items of all slots in table order, 256 consecutive
    items per block -> one partial per block."""
    return block_sum(_rows(np.concatenate([item_sums(g) for g in slots])))


def square_sum(slots):
    """Both stages: thread t of the one second-stage block adds partials t,
    t + 256, ... in that order onto 0.0, then the block sum."""
    rows = _rows(block_partials(slots))
    acc = np.zeros(THREADS, np.float64)
    for r in rows:
        acc = acc + r
    return float(block_sum(acc)[0])


def norm(slots):
    """The L2 norm over the fp32 tensors ``slots`` as ``norm_out`` holds it."""
    return float(np.sqrt(np.float64(square_sum(slots))))


def coef(norm_value, max_norm):
    """clip_grad_norm_'s coefficient in float64 (its 1e-6)."""
    with np.errstate(invalid="ignore"):       # inf / inf: NaN, as on the device
        q = np.float64(max_norm) / (np.float64(norm_value) + np.float64(1e-6))
    return float(1.0 if q > 1.0 else q)


def clipped(g, c):
    """The gradient as the clipped step stores it back."""
    return (np.asarray(g, np.float32).astype(np.float64) * np.float64(c)).astype(np.float32)
