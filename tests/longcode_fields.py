"""Arrays whose Huffman code book is a chain with a longest code word of exactly L bits (plain numpy; nothing of the library is used).

A Huffman code word of L bits needs at least F(L + 2) symbols (Fibonacci), so the arrays of the other test files (a few million smooth or noisy values)
stay near 12 bits, while the packing kernels change at 32.  The construction that gets there with the fewest values:

* the array holds integers and the bound is ABS 0.5, so every Lorenzo prediction, quantisation and reconstruction is exact in floating point and the code of
  a point is `radius +` the mixed difference of the array (one difference per axis);
* hence the residuals `r` are chosen freely and the array is their cumulative sum over every axis;
* the L rarest residual values get the counts c1 = 1, c2 = 2, c(i+2) = c(i+1) + c(i) + 1 (the `+ 1` removes the ties that exact Fibonacci numbers would hand
  to the heap's order), at random places; every other place holds residual 0, and there are at least c(L) + c(L-1) + 1 of those, so that 0 is the commonest
  symbol and the tree is one chain: L + 1 symbols, code lengths 1, 2, ..., L, L;
* the rare values take the large magnitudes, +-((L + 1) // 2) down to +-1, each value's sign chosen to cancel the running sum of count x value -- with the
  signs alternating naively that sum is not zero and the array drifts away (|x| = 5.7 million at L = 32), while float32 needs 8 |x| < 2^24: the Lorenzo sum has
  seven terms and every partial sum must stay exact.

With `quantization_intervals = 128` fixed (so that no interval optimiser folds the tail away) the radius is 64 and the codes are 64 + r."""
import numpy as np

BOUND = 0.5                  # ABS error bound the arrays are made for
INTERVALS = 128              # quantization_intervals the arrays are made for


def chain_counts(L):
    """c[0] is the rarest symbol's count; the counts of the L rare symbols."""
    c = [1, 2]
    while len(c) < L:
        c.append(c[-1] + c[-2] + 1)
    return c[:L]


def places_needed(L):
    """The fewest values an array must have for a longest code word of L bits."""
    c = chain_counts(L)
    return sum(c) + c[-1] + (c[-2] if L > 1 else 0) + 1


def places_for_leading_one(L):
    """In an array of the fewest places the chain's values together outweigh the zeros, so the root's lighter child (bit 1: Huffman.c:181) is the symbol 0 and
    every long code word is 0...0x -- its high bits are all zero, and a packer that lost them would not show.  With more than twice the chain's values in the
    array the chain is the lighter child: every long code word is 10...0x, the top bit of the longest set."""
    return 2 * sum(chain_counts(L)) + 1


def smallest_cube(L, not_multiple_of=None, leading_one=False):
    e = 2
    while e ** 3 < (places_for_leading_one(L) if leading_one else places_needed(L)) or (not_multiple_of and e % not_multiple_of == 0):
        e += 1
    return e


def chain_values(L):
    """The residual values of the L rare symbols, rarest first: magnitudes (L + 1) // 2 down to 1, the two ranks of a magnitude of opposite sign, which of them
    positive decided -- from the commonest down -- so that the sum of count x value stays near zero."""
    c = chain_counts(L)
    v = [0] * L
    run = 0
    j = L - 1
    while j >= 0:
        m = (L - 1 - j) // 2 + 1
        if j >= 1 and (L - j) // 2 + 1 == m:            # ranks j and j - 1 share the magnitude m
            d = m * (c[j] - c[j - 1])                    # what the pair adds when the commoner of the two is the positive one
            s = -1 if abs(run + d) > abs(run - d) else 1
            v[j], v[j - 1] = s * m, -s * m
            run += s * d
            j -= 2
        else:                                            # the odd one out: the rarest symbol of an odd L
            s = -1 if run > 0 else 1
            v[j] = s * m
            run += s * m * c[j]
            j -= 1
    return v


def longcode_residuals(L, n, seed):
    """n residuals (int16, flat): the chain's values at random places, 0 elsewhere."""
    c, v = chain_counts(L), chain_values(L)
    assert len(set(v)) == L and 0 not in v
    assert max(abs(x) for x in v) < INTERVALS // 2 - 1
    assert n >= places_needed(L), f"L = {L} needs {places_needed(L)} values, the array has {n}"
    total = sum(c)
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=np.int16)
    r[:total] = np.repeat(np.asarray(v, dtype=np.int16), c)
    rng.shuffle(r)
    # the SZ 1.4 path stores an array's first value (1-D: the first two) exactly, whatever it is: those places hold residual 0, so that no chain value loses a count
    for i in (0, 1):
        if r[i]:
            z = 2 + int(np.flatnonzero(r[2:4096] == 0)[0])
            r[i], r[z] = 0, r[i]
    assert int(np.count_nonzero(r)) == total and n - total >= c[-1] + (c[-2] if L > 1 else 0) + 1
    return r


def longcode_field(L, shape, dtype, seed, boxes=None):
    """An array of `shape` (1-D or 3-D) whose codes under ABS 0.5 and 128 intervals are 64 + r with r of the chain above: the longest code word has L bits.
    boxes = (b0, b1, b2): the cumulative sums start anew in every box of that size (the arrays of the OpenMP container, whose boxes are predicted on their own;
    boxes = shape: the array for the SZ 1.4 path in 3-D, which predicts as one such box).
    Asserts that the place count allows L bits and that every sum the prediction makes is exact in `dtype`."""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    r = longcode_residuals(L, n, seed).reshape(shape)
    x = r.astype(np.int32 if np.dtype(dtype) == np.float32 else np.int64)
    if boxes is None:
        for ax in range(x.ndim):
            np.cumsum(x, axis=ax, out=x)
    else:
        # The container predicts the first row of a box's first plane along the row alone -- its first value by itself (code = radius whatever the value: the
        # residual there must be 0, so a chain value that fell there changes places with a 0 of that row), the second from the first, the others from the two
        # before them (2 left - left-left): that row is the DOUBLE cumulative sum of its residuals.
        assert x.ndim == 3 and all(s % b == 0 for s, b in zip(shape, boxes)) and boxes[2] >= 8
        g = [s // b for s, b in zip(shape, boxes)]
        xb = x.reshape(g[0], boxes[0], g[1], boxes[1], g[2], boxes[2])
        rows = xb[:, 0, :, 0, :, :]                                      # (a view: the first rows of the boxes)
        for i, j, k in np.argwhere(rows[..., 0] != 0):
            z = 1 + int(np.flatnonzero(rows[i, j, k, 1:] == 0)[0])
            rows[i, j, k, 0], rows[i, j, k, z] = 0, rows[i, j, k, 0]
        np.cumsum(rows, axis=-1, out=rows)
        for ax in (1, 3, 5):
            np.cumsum(xb, axis=ax, out=xb)
    peak = int(np.abs(x).max())
    mant = 24 if np.dtype(dtype) == np.float32 else 53
    assert 8 * peak < 2 ** mant, f"|x| reaches {peak}: the prediction's sums are not exact in {np.dtype(dtype).name}"
    return np.ascontiguousarray(x.astype(dtype))


def expected_code_lengths(L):
    """{code: length} of the chain for the codes 64 + r; the commonest symbol (r = 0) has one bit, the two rarest L."""
    v = chain_values(L)
    out = {INTERVALS // 2: 1}
    for j in range(L):
        out[INTERVALS // 2 + v[j]] = min(L - j + 1, L)
    return out
