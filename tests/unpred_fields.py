"""Arrays for tests/test_unpredictable.py: unpredictable values (quantisation code 0, the original value in a list behind the Huffman payload) at chosen
densities, at exact counts per block column and at chosen places, and arrays whose code book has one or two symbols.

Every array is made for ABS 1e-3 and `quantization_intervals = max_quant_intervals = 32` (radius 16: a prediction error of 0.03 and more is unpredictable), and
every builder asks the ORACLE (tests/oracle_lib.py) what it made of the array -- the block-ordered codes, total_unpred, reg_count, the raw-store flag, the distinct
codes -- and asserts the property the array is built for.  A test that uses an array therefore fails on the precondition, it never passes vacuously.

Geometry (sz_amd/csrc/szh_geom.h): an axis of n values has n // 6 blocks, the first n % (n // 6) of them one value wider.  A block column is every block of one
(b0, b1); its codes are contiguous in block order.  k_permute cuts a column into segments of `perm_segb` blocks along the row (szhip_rt.inc, choose_segb).

Lorenzo prediction reads the reconstructed values of the seven neighbours behind a point; an unpredictable point is reconstructed as itself.  An outlier therefore
makes itself and its (up to) seven forward neighbours unpredictable, unless outliers happen to cancel in a neighbour's prediction: the exact-count builder plants,
asks the oracle for the codes, and goes on from what the oracle says."""
import numpy as np

BOUND = 1e-3
INTERVALS = 32
SZH_ZCAP = 128               # zero positions k_permute notes per (column, segment)      (sz_amd/csrc/szhip_kernels.h)
SZH_ZMAX = 1024              # zero codes of a column k_unpred orders by rank            (sz_amd/csrc/szhip_kernels.h)

_CACHE = {}                  # name -> case dict: built once a process, never changed


def params(oracle, with_regression=1):
    # (a fixed interval count is also what the config reader leaves in max_quant_intervals: conf.c:193-197)
    return oracle.default_params(with_regression=with_regression, quantization_intervals=INTERVALS, max_quant_intervals=INTERVALS)


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------------------------ geometry

def axis(n):
    """(starts, sizes) of the blocks of an axis of n values"""
    num = 1 if n <= 6 else n // 6
    late, split = n // num, n % num
    sizes = np.asarray([late + 1] * split + [late] * (num - split))
    return np.concatenate(([0], np.cumsum(sizes)[:-1])), sizes


def block_order(shape):
    """flat natural index of every place of the block-ordered code array (3-D)"""
    key = ("perm", tuple(shape))
    if key not in _CACHE:
        nat = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
        ax = [axis(n) for n in shape]
        parts = [nat[a:a + sa, b:b + sb, c:c + sc].reshape(-1) for a, sa in zip(*ax[0]) for b, sb in zip(*ax[1]) for c, sc in zip(*ax[2])]
        _CACHE[key] = np.concatenate(parts)
    return _CACHE[key]


def natural_codes(codes_blk, shape):
    out = np.empty(int(np.prod(shape)), dtype=np.int32)
    out[block_order(shape)] = codes_blk
    return out.reshape(shape)


def column_zeros(zero_mask):
    """zero codes per block column: an array (blocks along axis 0, blocks along axis 1)"""
    s0, s1 = axis(zero_mask.shape[0])[0], axis(zero_mask.shape[1])[0]
    return np.add.reduceat(np.add.reduceat(zero_mask.sum(axis=2), s0, axis=0), s1, axis=1)


def perm_segments(shape):
    """[k_begin, k_end) of the segments k_permute cuts a block column into (choose_segb with its 32 KB tile; at most 32 blocks)"""
    ax = [axis(n) for n in shape]
    per_block = int(ax[0][1][0]) * int(ax[1][1][0]) * int(ax[2][1][0]) * 2
    num = len(ax[2][0])
    segb = max(1, min(32 * 1024 // per_block, 32, num))
    ends = list(ax[2][0]) + [shape[2]]
    return [(int(ends[b]), int(ends[min(b + segb, num)])) for b in range(0, num, segb)]


# ------------------------------------------------------------------------------------------------------------------ the oracle's view of an array

def ask(oracle, x, with_regression=1):
    """What the oracle makes of a 3-D (or 2-D) array on the SZ 2.1 path: stream, decoded values, and the stages the builders assert on."""
    ref, st = oracle.compress(x, oracle.ABS, BOUND, params=params(oracle, with_regression), want_stages=True)
    raw = bool(ref[3] & 0x10)
    c = dict(x=x, ref=ref, raw=raw)
    if st is not None:
        assert st["intervals"] == INTERVALS
        c.update(codes=st["codes"], total_unpred=int(st["total_unpred"]), reg_count=int(st["reg_count"]), num_blocks=int(st["num_blocks"]),
                 distinct=np.unique(st["codes"]), huff_bytes=int(st["huff_bytes"]))
        assert int((st["codes"] == 0).sum()) == c["total_unpred"]
        if x.ndim == 3:
            c["zeros"] = natural_codes(st["codes"], x.shape) == 0
    return c


def finish(oracle, c):
    """the oracle's own decode: within the bound of the input, unpredictable points bit for bit; frozen"""
    x = c["x"]
    dec = oracle.decompress(c["ref"], x.shape, x.dtype)
    assert float(np.abs(dec.astype(np.float64) - x.astype(np.float64)).max()) <= BOUND
    if "zeros" in c:
        assert np.array_equal(bits(dec[c["zeros"]]), bits(x[c["zeros"]]))
    x.setflags(write=False); dec.setflags(write=False)
    c["dec"] = dec
    return c


# ------------------------------------------------------------------------------------------------------------------ (a) density arrays

# sigma -> (seed, band of the oracle's unpredictable fraction).  The bands are those the oracle gave for s_field + sigma N(0,1) at 24x32x48 and 20x30x42 (float32 and
# float64) when the arrays were designed; the seeds are ones with which every shape and type the tests build lies inside its band (profiles/r11_unpredictable.txt).
DENSITY = {3e-3: (1, (0.003, 0.005)), 8e-3: (8, (0.044, 0.061)), 2e-2: (21, (0.18, 0.19)), 1e-1: (4, (0.75, 0.76))}


def noisy(shape, sigma, dtype):
    from sz_amd.fields import s_field
    rng = np.random.default_rng(DENSITY[sigma][0])
    sh3 = (1,) * (3 - len(shape)) + tuple(shape)
    base = s_field(*sh3, np.float64).reshape(shape)
    return np.ascontiguousarray((base + sigma * rng.standard_normal(shape)).astype(dtype))


def density_case(oracle, shape, sigma, dtype=np.float32):
    """s_field + sigma N(0,1): the unpredictable fraction in the band of that sigma, not stored raw, every code of the alphabet in use"""
    key = ("density", tuple(shape), sigma, np.dtype(dtype).name)
    if key not in _CACHE:
        c = ask(oracle, noisy(shape, sigma, dtype))
        lo, hi = DENSITY[sigma][1]
        frac = c["total_unpred"] / c["x"].size
        assert not c["raw"], key
        assert lo <= frac <= hi, (key, frac)
        c["fraction"] = frac
        c["report"] = f"{shape} {np.dtype(dtype).name} sigma {sigma:g}: {c['total_unpred']} of {c['x'].size} unpredictable ({100 * frac:.2f} %), " \
                      f"{c['reg_count']} of {c['num_blocks']} regression blocks, {len(c['distinct'])} distinct codes, {len(c['ref'])} bytes"
        _CACHE[key] = finish(oracle, c)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------ (b) exact counts per block column

def base_case(oracle, shape, dtype=np.float32):
    """The smooth base: every block a Lorenzo block, no zero code.  0.7 x the S-field: at full scale the steps along the array's first edge (0.037 a value, predicted
    from one neighbour) are unpredictable under 32 intervals; at 0.3 and below some blocks take the regression."""
    from sz_amd.fields import s_field
    # (+- 5e-5 of seeded noise, a 20th of the bound: no two values of the base are equal, so an order error in the list of unpredictable values changes the stream)
    jitter = 1e-4 * (np.random.default_rng(13).random(shape) - 0.5)
    c = ask(oracle, np.ascontiguousarray((0.7 * s_field(*shape, np.float64) + jitter).astype(dtype)))
    assert c["reg_count"] == 0 and c["total_unpred"] == 0 and not c["raw"], (shape, c["reg_count"], c["total_unpred"])
    return c


def _outlier_values(shape, seed):
    """A distinct offset for every place: magnitude in [1, 2), either sign -- thirty times what the 32 intervals cover"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    v = 1.0 + (rng.permutation(n) + 0.5) / n
    return (v * rng.choice([-1.0, 1.0], size=n)).reshape(shape)


def _forward(p, shape):
    i, j, k = p
    return [(a, b, c) for a in (i, i + 1) for b in (j, j + 1) for c in (k, k + 1) if a < shape[0] and b < shape[1] and c < shape[2]]


def exact_count_case(oracle, shape, col, K, dtype=np.float32, krange=None, seed=7):
    """Exactly K zero codes in block column `col` = (b0, b1), none in any other column.  krange = (k0, k1): every one of them inside [k0, k1) along the row (one
    segment of the column).  Outliers go to the rows of the column that have a row behind them on both axes inside the column, so that no forward neighbour
    lies in another column: first a box of them (about K - 60 zeros), then one at a time, each chosen so that -- by the rule of the forward neighbours -- it adds
    as many zeros as still fit, and the oracle is asked after every one; an outlier that added too many (never seen: a cancellation would have to remove one
    first) is taken back."""
    key = ("exact", tuple(shape), col, K, np.dtype(dtype).name, krange)
    if key in _CACHE:
        return _CACHE[key]
    base = base_case(oracle, shape, dtype)["x"]
    off = _outlier_values(shape, seed).astype(dtype)
    (st0, sz0), (st1, sz1) = axis(shape[0]), axis(shape[1])
    i0, i1 = int(st0[col[0]]), int(st0[col[0]] + sz0[col[0]])
    j0, j1 = int(st1[col[1]]), int(st1[col[1]] + sz1[col[1]])
    k0, k1 = krange if krange is not None else (0, shape[2])
    klast = k1 - 1 if k1 < shape[2] else k1                      # outliers at k < klast: their forward neighbours stay below k1 (or the array ends there)
    rows = (i1 - i0) * (j1 - j0)
    assert K <= rows * (k1 - k0), (key, "the column does not hold that many codes")
    planted = np.zeros(shape, dtype=bool)

    def view():
        x = np.ascontiguousarray(np.where(planted, base + off, base).astype(dtype))
        c = ask(oracle, x)
        cz = column_zeros(c["zeros"])
        return c, int(cz[col]), int(cz.sum()) - int(cz[col])

    # the box: whole rows' worth of zeros, (rows) x (depth + 1)
    depth = max(0, (K - 60) // rows - 1)
    if depth:
        planted[i0:i1 - 1, j0:j1 - 1, k0:k0 + depth] = True
    c, have, elsewhere = view()
    assert elsewhere == 0 and have <= K, (key, have, elsewhere)
    cand = [(i, j, k) for k in range(k0, klast) for i in range(i0, i1 - 1) for j in range(j0, j1 - 1)]
    cand += [(i, j, k) for k in range(klast, k1) for i in range(i0, i1 - 1) for j in range(j0, j1 - 1)]     # (the array's last face: four forward neighbours)
    steps = tries = 0
    for p in cand:
        if have == K:
            break
        # (the rule of the forward neighbours, to pass over places that would add too many; a block that the outliers have turned into a regression block does not
        #  follow it -- there an outlier adds itself alone -- so the oracle decides)
        if planted[p] or (c["reg_count"] == 0 and sum(1 for q in _forward(p, shape) if not c["zeros"][q]) > K - have):
            continue
        planted[p] = True
        c2, have2, elsewhere = view()
        tries += 1
        assert tries <= 300, (key, have)
        if elsewhere or have2 > K or have2 <= have:
            planted[p] = False
            continue
        c, have, steps = c2, have2, steps + 1
    cz = column_zeros(c["zeros"])
    assert int(cz[col]) == K and int(cz.sum()) == K and c["total_unpred"] == K and not c["raw"], key
    zk = np.flatnonzero(c["zeros"][i0:i1, j0:j1].any(axis=(0, 1)))
    assert k0 <= zk.min() and zk.max() < k1, (key, zk.min(), zk.max())
    vals = c["x"][c["zeros"]]
    assert len(np.unique(bits(vals))) == K, (key, "the unpredictable values are not distinct: an order error in the list would not show")
    c["column_zeros"] = cz
    segs = perm_segments(shape)
    per_seg = [int(c["zeros"][i0:i1, j0:j1, a:b].sum()) for a, b in segs]
    c["report"] = f"{shape} {np.dtype(dtype).name} column {col} K = {K}: zeros per column {cz.tolist()}, per segment of the column {per_seg}, " \
                  f"{int(planted.sum())} outliers ({steps} placed singly), {c['reg_count']} regression blocks, {len(c['distinct'])} distinct codes"
    c["per_segment"] = per_seg
    _CACHE[key] = finish(oracle, c)
    return _CACHE[key]


def spread_count_case(oracle, shape, col, K, dtype=np.float32, seed=7):
    """Exactly K zero codes in block column `col`, none elsewhere, spread over ALL of k_permute's segments of the column with at most SZH_ZCAP = 128 in any of them:
    no segment's note overflows, so K alone decides k_unpred's route -- the ordered list up to SZH_ZMAX = 1024 (keys of several segments one behind the other), the
    scan beyond.  Every segment is first brought to (SZH_ZMAX - 9) // segments zeros (or up to seven fewer, where no place adds the last few) (that state is kept and shared by the K of one shape), then the segments
    take one more outlier each in turn, of as many zeros as still fit, until the column holds K."""
    key = ("spread", tuple(shape), col, K, np.dtype(dtype).name)
    if key in _CACHE:
        return _CACHE[key]
    segs = perm_segments(shape)
    base = base_case(oracle, shape, dtype)["x"]
    off = _outlier_values(shape, seed).astype(dtype)
    (st0, sz0), (st1, sz1) = axis(shape[0]), axis(shape[1])
    i0, i1 = int(st0[col[0]]), int(st0[col[0]] + sz0[col[0]])
    j0, j1 = int(st1[col[1]]), int(st1[col[1]] + sz1[col[1]])
    kstarts, ksizes = axis(shape[2])
    floor = (SZH_ZMAX - 9) // len(segs)                           # (the same for every K round the threshold: the state is shared)
    assert len(segs) >= 8 and floor + 8 <= SZH_ZCAP, (key, len(segs), floor)

    def view(planted):
        c = ask(oracle, np.ascontiguousarray(np.where(planted, base + off, base).astype(dtype)))
        return c, [int(c["zeros"][i0:i1, j0:j1, a:b].sum()) for a, b in segs]

    def grow(planted, c, per, sg, want, once=False):
        """outliers into segment sg until it holds `want` zeros (once: one outlier that adds any number up to that, if the first 40 places tried have one); every
        other segment and column as it was"""
        k0, k1 = segs[sg]
        klast = k1 - 1 if k1 < shape[2] else k1
        tries = 0
        for p in ((i, j, k) for k in range(k0, klast) for i in range(i0, i1 - 1) for j in range(j0, j1 - 1)):
            if per[sg] == want:
                break
            # (fewer than 8 wanted: only a place that is not zero yet, in a block the outliers have already turned into a regression block -- there an outlier adds
            #  itself alone, in a Lorenzo block its seven forward neighbours as well; the oracle decides either way)
            kb = int(np.searchsorted(kstarts, p[2], side="right")) - 1
            if planted[p] or c["zeros"][p] or (want - per[sg] < 8 and not c["zeros"][i0:i1, j0:j1, kstarts[kb]:kstarts[kb] + ksizes[kb]].any()):
                continue
            planted[p] = True
            c2, per2 = view(planted)
            tries += 1
            assert once or tries <= 120, (key, sg, per)
            if (once and tries > 40) or (not once and tries > 30 and per[sg] >= want - 7):
                planted[p] = False
                break
            if c2["total_unpred"] != sum(per2) or per2[:sg] + per2[sg + 1:] != per[:sg] + per[sg + 1:] or not per[sg] < per2[sg] <= want:
                planted[p] = False
                continue
            c, per = c2, per2
            if once:
                break
        assert once or want - 7 <= per[sg] <= want, (key, sg, per)
        return c, per

    skey = ("spread-floor", tuple(shape), col, floor, np.dtype(dtype).name)
    if skey not in _CACHE:
        planted = np.zeros(shape, dtype=bool)
        c, per = view(planted)
        for sg in range(len(segs)):
            c, per = grow(planted, c, per, sg, floor)
        _CACHE[skey] = (planted, c, per)
    planted, c, per = _CACHE[skey]
    planted, per = planted.copy(), list(per)
    for visit in range(12 * len(segs)):
        if sum(per) == K:
            break
        sg = visit % len(segs)
        c, per = grow(planted, c, per, sg, per[sg] + min(K - sum(per), 8), once=True)
    cz = column_zeros(c["zeros"])
    assert int(cz[col]) == K and int(cz.sum()) == K and c["total_unpred"] == K and not c["raw"], key
    assert max(per) <= SZH_ZCAP and sum(1 for q in per if q) >= 8, (key, per)          # the precondition: no segment's note overflows, many segments hold zeros
    assert len(np.unique(bits(c["x"][c["zeros"]]))) == K, (key, "the unpredictable values are not distinct: an order error in the list would not show")
    c["column_zeros"], c["per_segment"] = cz, per
    c["report"] = f"{shape} {np.dtype(dtype).name} column {col} K = {K} spread: zeros per column {cz.tolist()}, per segment of the column {per}, " \
                  f"{int(planted.sum())} outliers, {c['reg_count']} regression blocks, {len(c['distinct'])} distinct codes"
    _CACHE[key] = finish(oracle, c)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------ (c) zero codes at chosen places

def position_case(oracle, shape, places, name, dtype=np.float32, full_column=None, seed=11):
    """The base with an outlier at every place of `places` (and at every point of block column `full_column`): the oracle's codes are zero at each of them."""
    key = ("position", name, np.dtype(dtype).name)
    if key in _CACHE:
        return _CACHE[key]
    base = base_case(oracle, shape, dtype)["x"]
    off = _outlier_values(shape, seed).astype(dtype)
    planted = np.zeros(shape, dtype=bool)
    for p in places:
        planted[tuple(np.asarray(p) % np.asarray(shape))] = True           # (negative indices count from the end)
    if full_column is not None:
        (st0, sz0), (st1, sz1) = axis(shape[0]), axis(shape[1])
        b0, b1 = full_column
        planted[st0[b0]:st0[b0] + sz0[b0], st1[b1]:st1[b1] + sz1[b1], :] = True
    c = ask(oracle, np.ascontiguousarray(np.where(planted, base + off, base).astype(dtype)))
    assert not c["raw"] and bool(c["zeros"][planted].all()), (name, "an outlier's code is not zero")
    c["column_zeros"] = column_zeros(c["zeros"])
    c["report"] = f"{name} {shape} {np.dtype(dtype).name}: {c['total_unpred']} unpredictable, zeros per column {c['column_zeros'].tolist()}, " \
                  f"{c['reg_count']} regression blocks, {len(c['distinct'])} distinct codes"
    _CACHE[key] = finish(oracle, c)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------ (d) code books of one and two symbols

def plane(shape, dtype):
    """An exact plane (small integer coefficients on integer indices: exact in float32): every block a regression block that predicts every point exactly"""
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return np.ascontiguousarray(sum((q + 1) * 0.25 * a for q, a in enumerate(g)).astype(dtype))


def book_case(oracle, name, x, symbols):
    """An array whose codes take exactly `symbols` distinct values (1: all the radius, no payload bit)."""
    key = ("book", name)
    if key not in _CACHE:
        c = ask(oracle, x)
        assert not c["raw"] and len(c["distinct"]) == symbols, (name, c["distinct"])
        if symbols == 1:
            assert c["distinct"][0] == INTERVALS // 2 and c["huff_bytes"] == 0 and c["total_unpred"] == 0, (name, c["distinct"], c["huff_bytes"])
        c["report"] = f"{name} {x.shape} {x.dtype.name}: distinct codes {c['distinct'].tolist()}, {c['reg_count']} of {c['num_blocks']} regression blocks, " \
                      f"huff_bytes {c['huff_bytes']}, {c['total_unpred']} unpredictable"
        _CACHE[key] = finish(oracle, c)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------ the other formats

OMP_META = bytes(range(1, 33))
OMP_THREADS = 8              # 2 x 2 x 2 boxes of 16^3 in a 32^3 array
BAND_LOW, BAND_HIGH = (0.044, 0.061), (0.75, 0.76)

# format -> (kind, shape, sigma for the 4 - 6 % band, sigma for the 75 % band): each format predicts in its own way, so each has its own noise level for a band; the
# sigmas were found by bisection against the oracle, and the oracle's fraction is asserted to lie in the band every time the array is built
FORMATS = {"sz21-2d": ("sz21", (60, 72), 7.7e-3, 1e-1), "sz14-3d": ("sz14", (20, 30, 42), 5.6e-3, 3.7e-2), "sz14-2d": ("sz14", (60, 72), 8.1e-3, 4.9e-2),
           "sz14-1d": ("sz14", (4000,), 9.7e-3, 7e-2), "omp": ("omp", (32, 32, 32), 5.9e-3, 3.8e-2)}


def omp_params(oracle):
    p = oracle.default_params()
    p.quantization_intervals = INTERVALS
    return p


def _omp_verbatim(ref, x):
    """unpredictable values per box, read from the container (sz_omp.c: box count, a value, intervals, tree bytes, node count, the tree, a count per box)"""
    q = len(OMP_META)
    nb = int.from_bytes(ref[q:q + 4], "big"); q += 4 + x.dtype.itemsize
    intervals, tree_bytes = int.from_bytes(ref[q:q + 4], "big"), int.from_bytes(ref[q + 4:q + 8], "big"); q += 12 + tree_bytes
    assert nb == OMP_THREADS and intervals == INTERVALS
    return np.frombuffer(ref, np.uint32, nb, q).astype(np.int64)


def format_ask(oracle, kind, x):
    """dict(x, ref, dec, n_unpred, raw) of the oracle for an array in one of the other formats (kind: sz21 | sz14 | omp)"""
    x = np.ascontiguousarray(x)
    c = dict(x=x, kind=kind)
    if kind == "omp":
        c["ref"] = oracle.omp_compress(x, BOUND, OMP_THREADS, OMP_META, omp_params(oracle))
        c["per_box"] = _omp_verbatim(c["ref"], x)
        c["n_unpred"], c["raw"] = int(c["per_box"].sum()), False
        c["dec"] = oracle.omp_decompress(c["ref"], len(OMP_META), x.shape, x.dtype)
    else:
        sz14 = kind == "sz14" or x.ndim == 1
        ref, st = oracle.compress(x, oracle.ABS, BOUND, params=params(oracle, 0 if sz14 else 1), want_stages=True)
        c["ref"], c["raw"] = ref, bool(ref[3] & 0x10)
        assert st is not None and st["intervals"] == INTERVALS
        c["n_unpred"] = int(st["exact_count"] if sz14 else st["total_unpred"])
        c["codes"] = st["codes"]                                                       # (SZ 1.4: natural order; SZ 2.1 2-D: block order)
        assert int((st["codes"] == 0).sum()) == c["n_unpred"]
        c["dec"] = oracle.decompress(ref, x.shape, x.dtype)
    assert float(np.abs(c["dec"].astype(np.float64) - x.astype(np.float64)).max()) <= BOUND
    x.setflags(write=False); c["dec"].setflags(write=False)
    return c


def format_density_case(oracle, fmt, high, dtype=np.float32):
    key = ("format", fmt, high, np.dtype(dtype).name)
    if key not in _CACHE:
        from sz_amd.fields import s_field
        kind, shape, s_low, s_high = FORMATS[fmt]
        sigma, band, seed = (s_high, BAND_HIGH, 4) if high else (s_low, BAND_LOW, 2)
        sh3 = (1,) * (3 - len(shape)) + tuple(shape)
        x = (s_field(*sh3, np.float64).reshape(shape) + sigma * np.random.default_rng(seed).standard_normal(shape)).astype(dtype)
        c = format_ask(oracle, kind, x)
        frac = c["n_unpred"] / x.size
        assert not c["raw"] and band[0] <= frac <= band[1], (key, frac, c["raw"])
        c["report"] = f"{fmt} {shape} {np.dtype(dtype).name} sigma {sigma:g}: {c['n_unpred']} of {x.size} unpredictable ({100 * frac:.2f} %), {len(c['ref'])} bytes"
        _CACHE[key] = c
    return _CACHE[key]


def format_position_case(oracle, fmt, dtype=np.float32):
    """The smooth base of the format's shape with outliers at the first and last element, at both ends of a row and (3-D) in the last row of a box / of the array."""
    key = ("format-position", fmt, np.dtype(dtype).name)
    if key not in _CACHE:
        from sz_amd.fields import s_field
        kind, shape = FORMATS[fmt][:2]
        sh3 = (1,) * (3 - len(shape)) + tuple(shape)
        jitter = 1e-4 * (np.random.default_rng(13).random(shape) - 0.5)
        x = (0.7 * s_field(*sh3, np.float64).reshape(shape) + jitter).astype(dtype)
        off = _outlier_values(shape, 17).astype(dtype)
        places = {1: [(0,), (-1,), (1234,), (1235,)],
                  2: [(0, 0), (-1, -1), (7, 0), (7, -1), (30, 11), (-1, 40)],
                  3: [(0, 0, 0), (-1, -1, -1), (7, 9, 0), (7, 9, -1), (15, 15, 15), (16, 16, 16), (-1, 20, 6), (9, -1, 30)]}[len(shape)]
        mask = np.zeros(shape, dtype=bool)
        for p in places:
            mask[p] = True
        x[mask] += off[mask]
        c = format_ask(oracle, kind, x)
        assert not c["raw"] and c["n_unpred"] >= len(places), (key, c["n_unpred"])
        if kind == "omp":
            assert c["per_box"][0] > 0 and c["per_box"][-1] > 0, (key, c["per_box"])
        elif kind == "sz14" or len(shape) == 1:
            assert bool((c["codes"].reshape(shape)[mask] == 0).all()), (key, "an outlier's code is not zero")
        c["report"] = f"{fmt} {shape} {np.dtype(dtype).name} places: {c['n_unpred']} unpredictable" + (f", per box {c['per_box'].tolist()}" if kind == "omp" else "")
        _CACHE[key] = c
    return _CACHE[key]
