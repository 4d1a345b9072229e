"""numpy restatement of the shuffled-minibatch mode: the
permutation kernel of libmarlnav.so ``marlnav_minibatch_permutations`` bit for
bit, the cut of an epoch's permutation into minibatches, and the physically
gathered buffer that is the oracle of the gather kernels.

The permutation of epoch e at call counter c, seed s, network tag n over L
steps (include/marlnav.h): a Fisher-Yates over the identity, for i = L - 1
down to 1 draw number d = L - 1 - i is word d & 1 of Philox2x32-10 with the
counter words (e << 16 | d >> 1, lo32(c)) under the key native_key(mix(s),
0x5045524D + n, c); j = word * (i + 1) >> 32; positions i and j are swapped.
"""
import numpy as np
import torch

from policy_ref import _M32, _M64, native_key, philox2x32_10, seed_mix

PERM_BLOCK = 0x5045524D
MAX_STEPS = 65535
ACTOR, CRITIC = 0, 1


def permutations(L, E, seed, network, counter=0, epochs=None):
    """The (E, L) int32 table the kernel writes for call counter ``counter``.
    ``epochs``: the rows wanted (default all E), for sampling many epochs."""
    L, E, c = int(L), int(E), int(counter) & _M64
    assert 1 <= L <= MAX_STEPS and 1 <= E <= MAX_STEPS
    key = native_key(seed_mix(int(seed) & _M64), (PERM_BLOCK + int(network)) & _M32, c)
    ep = np.arange(E, dtype=np.uint64) if epochs is None else np.asarray(epochs, np.uint64)
    table = np.tile(np.arange(L, dtype=np.int32), (len(ep), 1))
    draws = L - 1
    if draws == 0:
        return table
    nblk = (draws + 1) // 2
    c0 = (ep[:, None] << np.uint64(16)) | np.arange(nblk, dtype=np.uint64)[None, :]
    c1 = np.full_like(c0, c & _M32)
    w0, w1 = philox2x32_10(c0, c1, key)
    words = np.stack([w0, w1], axis=2).reshape(len(ep), 2 * nblk).astype(np.uint64)
    rows = np.arange(len(ep))
    for d in range(draws):
        i = L - 1 - d
        j = ((words[:, d] * np.uint64(i + 1)) >> np.uint64(32)).astype(np.int64)
        a, b = table[rows, i].copy(), table[rows, j].copy()
        table[rows, i], table[rows, j] = b, a
    return table


def minibatch_sizes(L, bs):
    """L // bs minibatches of bs steps, the last one with the L % bs left over."""
    n = L // bs
    if n == 0:
        raise ValueError("no minibatch")
    return [bs] * (n - 1) + [L - (n - 1) * bs]


def minibatches(perm, bs):
    """One epoch's minibatches: ``perm`` cut by ``minibatch_sizes``."""
    out, at = [], 0
    for n in minibatch_sizes(len(perm), bs):
        out.append([int(x) for x in perm[at:at + n]])
        at += n
    return out


def gathered(data, steps):
    """``data`` (the stacked (T, ...) tensors of a case) with its storage
    physically gathered: step slot s of the result is step ``steps[s]``."""
    idx = torch.as_tensor(list(steps), dtype=torch.int64)
    return {k: v.index_select(0, idx.to(v.device)) for k, v in data.items()}
