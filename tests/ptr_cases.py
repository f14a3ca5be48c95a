"""Helpers of tests/test_device_pointers.py: regions carved out of a larger allocation at a chosen byte offset, with guard bytes all round, and the
arrays / oracle results the cases share.  One implementation serves torch uint8 tensors on the GPU and numpy arrays for the CPU shim (where "device"
memory is host memory)."""
import numpy as np

FILL = 0xA5
ALIGN = 256


class Region:
    """`nbytes` bytes at `ptr` = (a 256-byte aligned address inside the allocation) + 256 + off.  Everything else of the allocation is guard."""

    def __init__(self, whole, addr, start, nbytes, device):
        self.whole, self.start, self.nbytes, self.device = whole, start, nbytes, device
        self.ptr = addr + start

    def _host(self, a, b):
        part = self.whole[a:b]
        return part.cpu().numpy() if self.device else part.copy()

    def put(self, data, at=0):
        """copy an array's (or a bytes object's) bytes into the region, from its byte `at` on"""
        u8 = np.frombuffer(data, dtype=np.uint8).copy() if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).reshape(-1).view(np.uint8).copy()
        assert at + u8.size <= self.nbytes
        a = self.start + at
        if self.device:
            import torch
            self.whole[a:a + u8.size].copy_(torch.from_numpy(u8))
            torch.cuda.synchronize()          # (the library's streams are non-blocking: what it reads must be complete when the call is made)
        else:
            self.whole[a:a + u8.size] = u8
        return self

    def get(self, n=None, at=0):
        """the region's bytes [at, at + n) as a numpy uint8 array (a copy)"""
        n = self.nbytes - at if n is None else n
        assert at + n <= self.nbytes
        return self._host(self.start + at, self.start + at + n)

    def check(self, what=""):
        """every byte in front of the region and behind its end still holds the fill byte"""
        front, back = self._host(0, self.start), self._host(self.start + self.nbytes, len(self.whole))
        for name, g, origin in (("in front of", front, -len(front)), ("behind", back, self.nbytes)):
            bad = np.nonzero(g != FILL)[0]
            assert bad.size == 0, (f"{what}: {bad.size} guard bytes {name} the region were written; the first at region byte {origin + int(bad[0])} "
                                   f"(region of {self.nbytes} bytes at ...{self.ptr & 0xfff:03x}) now holds 0x{int(g[bad[0]]):02x}")


def carve(nbytes, off=0, pad=4096, device=False):
    """A region of `nbytes` bytes, `off` bytes behind a 256-byte aligned address, `pad` guard bytes behind it (and at least 256 in front).  The aligned
    address is computed from the allocation's own address -- no allocator is trusted for it -- and the whole allocation is filled with 0xA5."""
    total = (ALIGN - 1) + ALIGN + off + nbytes + pad
    if device:
        import torch
        whole = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        addr = whole.data_ptr()
        torch.cuda.synchronize()
    else:
        whole = np.full(total, FILL, dtype=np.uint8)
        addr = whole.ctypes.data
    start = (-addr) % ALIGN + ALIGN + off
    r = Region(whole, addr, start, nbytes, device)
    assert (r.ptr - off) % ALIGN == 0 and start >= ALIGN and total - start - nbytes >= pad
    return r


# ------------------------------------------------------------------------------------------------------------------ arrays and the oracle's results

def _series(n):
    return np.ascontiguousarray((np.cumsum(np.random.default_rng(7).standard_normal(n)) * 0.01).astype(np.float32))


def _array(name):
    from sz_amd.fields import m_field, plane_field, s_field
    f64 = np.float64
    return {"s24x40x56": lambda: (s_field(24, 40, 56), 1e-3),                 # rows a multiple of 8 values
            "s14x20x36": lambda: (s_field(14, 20, 36), 1e-3),                 # rows = 4 mod 8
            "s14x19x33": lambda: (s_field(14, 19, 33), 1e-3),                 # odd rows: a control, the beam never takes it
            "m40": lambda: (m_field(40), 1e-4),                               # regression blocks, k_reg_points
            "m40-f64": lambda: (m_field(40, f64), 1e-5),
            "s20x24x40-f64": lambda: (s_field(20, 24, 40, f64), 1e-6),
            "plane70x90": lambda: (plane_field(70, 90), 1e-3),                # 2-D: shape (0, 70, 90) to the C ABI
            "sixty": lambda: (s_field(12, 16, 24), 5e-5),                     # tests/test_device_book.py's 12x16x24-float32-sixty: Lorenzo only
            "s20x24x40": lambda: (s_field(20, 24, 40), 1e-4),                 # SZ 1.4
            "series4097": lambda: (_series(4097), 1e-4),
            "omp-s64-t8": lambda: (s_field(64, 64, 64), 1e-4),                # 32^3 boxes: k_omp_col
            "omp-s8x8x18-t4": lambda: (s_field(8, 8, 18), 1e-3),
            "omp-s16x24x40-t16": lambda: (s_field(16, 24, 40), 1e-3)}[name]()


SZ21 = ["s24x40x56", "s14x20x36", "s14x19x33", "m40", "m40-f64", "s20x24x40-f64", "plane70x90"]
SZ14 = ["s20x24x40", "plane70x90", "series4097"]
OMP = {"omp-s64-t8": 8, "omp-s8x8x18-t4": 4, "omp-s16x24x40-t16": 16}
OMP_META = bytes(range(1, 33))
_REF = {}        # (kind, name) -> dict(x, eb, ref, dec): computed once, never changed


def shape3(x):
    """(r0, r1, r2) of the C ABI: r0 == 0 a 2-D array, r0 == r1 == 0 a 1-D array"""
    return (0,) * (3 - x.ndim) + tuple(x.shape)


def meta_len(x):
    return 4 + (28 if x.dtype == np.float32 else 36)


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def reference(oracle, name, kind="sz21"):
    """The oracle's stream of an array and what the oracle's decoder makes of it.  kind: sz21 | sz14 | omp"""
    key = (kind, name)
    if key not in _REF:
        x, eb = _array(name)
        x = np.ascontiguousarray(x)
        if kind == "omp":
            ref = oracle.omp_compress(x, eb, OMP[name], OMP_META)
            dec = oracle.omp_decompress(ref, len(OMP_META), x.shape, x.dtype)
        else:
            ref, _ = oracle.compress(x, oracle.ABS, eb, params=oracle.default_params(with_regression=0 if kind == "sz14" else 1))
            dec = oracle.decompress(ref, x.shape, x.dtype)
        x.setflags(write=False); dec.setflags(write=False)
        _REF[key] = dict(x=x, eb=eb, ref=ref, dec=dec)
    return _REF[key]


def beam_eligible(x):
    """beam_applies of sz_amd/csrc/szhip_rt.inc without its address test: a 3-D array whose rows are a multiple of four values"""
    return x.ndim == 3 and x.shape[2] >= 4 and x.shape[2] % 4 == 0


def expected_sweep(x, ptr):
    """stats.quant_kernel of an SZ 2.1 call on array x at address ptr: 2 (k_beam) needs 16-byte aligned rows, else 0 (k_pencil)"""
    return 2 if beam_eligible(x) and ptr % 16 == 0 else 0
