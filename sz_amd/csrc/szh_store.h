// szh_store.h -- the copy-shaped passes of the drop-in calls for device-resident arrays (include/sz.h: SZ_hip_compress_device, SZ_hip_decompress_device):
//   k_store_be   the raw store of SZ_compress_args_float_StoreOriData (sz/src/sz_float.c:526-552; doubles sz_double.c): n values -> big-endian bytes
//   k_load_be    its inverse (szd_float.c:106-118)
//   k_fill       the constant stream's decode (szd_float.c:96-104)
//   k_clamp      protectValueRange (szd_float.c:161-176)
// One shape for all four: the n values are cut at the 16-byte boundaries of the OUTPUT -- a head of fewer than 16 bytes up to the first boundary, whole 16-byte
// pieces (one store each; the input is read 16 bytes at a time where its address is aligned alike, else value by value), a tail behind the last boundary; head
// and tail go value by value.  Lanes take pieces grid-stride, consecutive lanes consecutive pieces.  Nothing in front of or behind the n values is written, the
// input is never written.  A BYTE address that is not aligned to the element (a stream in a caller's buffer that starts anywhere) is written / read byte by byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

template <class T> struct szh_be;
template <> struct szh_be<float> {
    typedef unsigned U;
    static __device__ __forceinline__ U swap(U u) { return __builtin_bswap32(u); }
};
template <> struct szh_be<double> {
    typedef unsigned long long U;
    static __device__ __forceinline__ U swap(U u) { return __builtin_bswap64(u); }
};
template <class T> __device__ __forceinline__ typename szh_be<T>::U szh_bits_of(T v) { typename szh_be<T>::U u; __builtin_memcpy(&u, &v, sizeof(T)); return u; }
template <class T> __device__ __forceinline__ T szh_value_of(typename szh_be<T>::U u) { T v; __builtin_memcpy(&v, &u, sizeof(T)); return v; }

// the cut of n values at the 16-byte boundaries of `anchor` (aligned to its element): [0, head) and [tail0, n) value by value, `pieces` 16-byte pieces between
template <class T> struct szh_cut {
    int64_t head, pieces, tail0;
    __device__ __forceinline__ szh_cut(const void *anchor, int64_t n)
    {
        constexpr int VW = 16 / (int)sizeof(T);
        head = (int64_t)(((16u - (unsigned)((uintptr_t)anchor & 15u)) & 15u) / (unsigned)sizeof(T));
        if (head > n) head = n;
        pieces = (n - head) / VW;
        tail0 = head + pieces * VW;
    }
};

// value i of the array as the stream holds it: byte-swapped, a zero replaced by `repl` first when the caller asks for it (the MSST19 raw copy, sz_float_pwr.c:2053-2058)
template <class T> __device__ __forceinline__ typename szh_be<T>::U szh_be_of(T v, int use_repl, T repl)
{
    if (use_repl && v == 0) v = repl;
    return szh_be<T>::swap(szh_bits_of<T>(v));
}

template <class T>
__global__ __launch_bounds__(256) void k_store_be(const T *__restrict__ src, unsigned char *__restrict__ dst, int64_t n, int use_repl, T repl)
{
    typedef typename szh_be<T>::U U;
    constexpr int VW = 16 / (int)sizeof(T);
    const int64_t lane = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x, lanes = (int64_t)gridDim.x * 256;
    if (((uintptr_t)dst & (sizeof(T) - 1)) != 0) {                  // the stream starts between element boundaries: byte stores
        for (int64_t i = lane; i < n; i += lanes) {
            const U u = szh_be_of<T>(src[i], use_repl, repl);
            unsigned char *q = dst + i * (int64_t)sizeof(T);
            for (int b = 0; b < (int)sizeof(T); ++b) q[b] = (unsigned char)(u >> (8 * b));
        }
        return;
    }
    U *d = reinterpret_cast<U *>(dst);
    const szh_cut<T> c(dst, n);
    if (lane < c.head) d[lane] = szh_be_of<T>(src[lane], use_repl, repl);
    if (lane < n - c.tail0) d[c.tail0 + lane] = szh_be_of<T>(src[c.tail0 + lane], use_repl, repl);
    const bool src16 = (((uintptr_t)(src + c.head)) & 15u) == 0;
    for (int64_t p = lane; p < c.pieces; p += lanes) {
        const int64_t j0 = c.head + p * VW;
        T t[VW]; U u[VW];
        if (src16) { const uint4 v = *reinterpret_cast<const uint4 *>(src + j0); __builtin_memcpy(t, &v, 16); }
        else for (int q = 0; q < VW; ++q) t[q] = src[j0 + q];
        for (int q = 0; q < VW; ++q) u[q] = szh_be_of<T>(t[q], use_repl, repl);
        uint4 o; __builtin_memcpy(&o, u, 16);
        *reinterpret_cast<uint4 *>(d + j0) = o;
    }
}

// element i of a big-endian stream at any byte address
template <class T> __device__ __forceinline__ T szh_load_be_at(const unsigned char *src, int64_t i, bool src_elem)
{
    typedef typename szh_be<T>::U U;
    U u;
    if (src_elem) u = reinterpret_cast<const U *>(src)[i];
    else { u = 0; const unsigned char *q = src + i * (int64_t)sizeof(T); for (int b = 0; b < (int)sizeof(T); ++b) u |= (U)q[b] << (8 * b); }
    return szh_value_of<T>(szh_be<T>::swap(u));
}

template <class T>
__global__ __launch_bounds__(256) void k_load_be(const unsigned char *__restrict__ src, T *__restrict__ dst, int64_t n)
{
    typedef typename szh_be<T>::U U;
    constexpr int VW = 16 / (int)sizeof(T);
    const int64_t lane = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x, lanes = (int64_t)gridDim.x * 256;
    const bool src_elem = ((uintptr_t)src & (sizeof(T) - 1)) == 0;
    const szh_cut<T> c(dst, n);
    if (lane < c.head) dst[lane] = szh_load_be_at<T>(src, lane, src_elem);
    if (lane < n - c.tail0) dst[c.tail0 + lane] = szh_load_be_at<T>(src, c.tail0 + lane, src_elem);
    const bool src16 = (((uintptr_t)(src + c.head * (int64_t)sizeof(T))) & 15u) == 0;
    for (int64_t p = lane; p < c.pieces; p += lanes) {
        const int64_t j0 = c.head + p * VW;
        T t[VW];
        if (src16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + j0 * (int64_t)sizeof(T));
            U u[VW]; __builtin_memcpy(u, &v, 16);
            for (int q = 0; q < VW; ++q) t[q] = szh_value_of<T>(szh_be<T>::swap(u[q]));
        } else
            for (int q = 0; q < VW; ++q) t[q] = szh_load_be_at<T>(src, j0 + q, src_elem);
        uint4 o; __builtin_memcpy(&o, t, 16);
        *reinterpret_cast<uint4 *>(dst + j0) = o;
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_fill(T *__restrict__ dst, int64_t n, T value)
{
    constexpr int VW = 16 / (int)sizeof(T);
    const int64_t lane = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x, lanes = (int64_t)gridDim.x * 256;
    const szh_cut<T> c(dst, n);
    if (lane < c.head) dst[lane] = value;
    if (lane < n - c.tail0) dst[c.tail0 + lane] = value;
    T t[VW];
    for (int q = 0; q < VW; ++q) t[q] = value;
    uint4 o; __builtin_memcpy(&o, t, 16);
    for (int64_t p = lane; p < c.pieces; p += lanes) *reinterpret_cast<uint4 *>(dst + c.head + p * VW) = o;
}

// szd_float.c:161-176: `if (v <= max && v >= min) continue; if (v < min) v = min; else if (v > max) v = max;` -- a NaN fails every comparison and stays
template <class T> __device__ __forceinline__ T szh_clamped(T v, T mn, T mx)
{
    if (v <= mx && v >= mn) return v;
    if (v < mn) return mn;
    if (v > mx) return mx;
    return v;
}

template <class T>
__global__ __launch_bounds__(256) void k_clamp(T *data, int64_t n, T mn, T mx)
{
    constexpr int VW = 16 / (int)sizeof(T);
    const int64_t lane = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x, lanes = (int64_t)gridDim.x * 256;
    const szh_cut<T> c(data, n);
    if (lane < c.head) data[lane] = szh_clamped<T>(data[lane], mn, mx);
    if (lane < n - c.tail0) data[c.tail0 + lane] = szh_clamped<T>(data[c.tail0 + lane], mn, mx);
    for (int64_t p = lane; p < c.pieces; p += lanes) {
        uint4 *at = reinterpret_cast<uint4 *>(data + c.head + p * VW);
        uint4 v = *at;
        T t[VW]; __builtin_memcpy(t, &v, 16);
        for (int q = 0; q < VW; ++q) t[q] = szh_clamped<T>(t[q], mn, mx);
        __builtin_memcpy(&v, t, 16);
        *at = v;
    }
}
