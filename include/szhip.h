/*
 * szhip.h -- C ABI of the MI355X (gfx950) HIP layer of the SZ 2.1 hot path.
 *
 * Everything below is `extern "C"`, plain pointers and sizes, no globals: this is what the
 * reference's own host code would bind instead of its CPU loops.  The reference has no FFI for
 * this path (it is one C library); the entry points therefore replace these internal call sites:
 *
 *   szhip_compress()      replaces  SZ_compress_float_3D_MDQ_nonblocked_with_blocked_regression
 *                                   (sz/src/sz_float.c:6527-7489) and the double twin
 *                                   (sz/src/sz_double.c:5904), called from SZ_compress_args_float
 *                                   (sz/src/sz_float.c:2974,3012) / _double
 *   szhip_decompress()    replaces  decompressDataSeries_float_3D_nonblocked_with_blocked_regression
 *                                   (sz/src/szd_float.c:3483-5866) / _double (szd_double.c:3316),
 *                                   called from SZ_decompress_args_float (sz/src/szd_float.c:133)
 *   szhip_minmax()        replaces  computeRangeSize_float/_double (sz/src/dataCompression.c:102,149)
 *
 * The streams produced/consumed are the reference's SZ 2.1 "raBytes" streams, byte for byte
 * (pre-lossless, i.e. what the reference emits with szMode = SZ_BEST_SPEED).
 */
#ifndef SZHIP_H
#define SZHIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SZHIP_OK            0
#define SZHIP_ERR_NODEVICE -1   /* no HIP device / runtime failure */
#define SZHIP_ERR_ARG      -2
#define SZHIP_ERR_UNSUP    -3   /* valid SZ input this layer does not cover yet */
#define SZHIP_ERR_STREAM   -4   /* malformed compressed stream */
#define SZHIP_ERR_INTERNAL -5   /* kernel-side timeout or inconsistency */
#define SZHIP_CONSTANT      1   /* szhip_compress with SZHIP_RANGE_FROM_DATA: max - min <= eb, nothing was encoded (stats.vmin / vmax are
                                   set, *out stays NULL): the caller writes the reference's constant-data stream (sz_float.c:2861) */

#define SZHIP_F32 0
#define SZHIP_F64 1

typedef struct szhip_ctx szhip_ctx; /* owns one HIP stream and grow-only device workspaces */

/* parameters the hot path reads from sz_params / sz_exedata (sz/include/sz.h:164-217), passed by value */
typedef struct szhip_params {
    int      sample_distance;        /* sampleDistance */
    float    pred_threshold;         /* predThreshold */
    unsigned max_quant_intervals;    /* max_quant_intervals (maxRangeRadius = half of it) */
    unsigned quantization_intervals; /* 0: optimise (optQuantMode 1); else fixed capacity */
    unsigned flags;                  /* SZHIP_RANGE_FROM_DATA: szhip_compress takes the array's value range from its own fit pass
                                        (one read of the input less than szhip_minmax + szhip_compress) and writes it into the
                                        range field of the parameter bytes in `meta` (min at +20, max = min + range, sz_float.c:2849);
                                        szhip_stats.vmin / vmax report it.  For callers whose bound does not depend on the range
                                        (ABS).  0: `meta` is used as given. */
} szhip_params;
#define SZHIP_RANGE_FROM_DATA 1u

/* per-call measurements (all times in milliseconds, device events on the ctx stream) */
typedef struct szhip_stats {
    double ms_total;        /* whole call, device side incl. host glue between kernels */
    double ms_prequant;     /* fit + sampling + selection kernels */
    double ms_quant;        /* the predict+quantise (or reconstruct) wavefront kernel alone */
    double ms_entropy;      /* histogram/permute/encode (or decode/permute) kernels */
    double ms_host;         /* host glue: tree build, coefficient chain, header */
    uint64_t n_elements, n_blocks, n_reg_blocks, n_unpred;
    unsigned intervals; int use_mean;
    uint64_t out_bytes;
    uint64_t quant_kernel_launches; /* launches of the wavefront kernel (1 per call) */
    double vmin, vmax;      /* the array's range when SZHIP_RANGE_FROM_DATA was set (else 0) */
    int chain_overlapped;   /* 1: the regression-coefficient chain ran next to the wavefront kernel */
    int quant_kernel;       /* which mapping of the wavefront kernel ran: 0 = k_pencil (8x8 pencils), 2 = k_beam (szh_beam.h); the OpenMP container: 3 = k_omp_col (32 x 32 box faces, 16-byte aligned array), 4 = k_omp_box reading rows 16 bytes at a time, 5 = k_omp_box value by value */
    int packing;            /* (round 6) 1: the Huffman packing read the sweep's natural-order codes segment by segment (szh_segenc.h); 0: block-ordered copy first.
                               The batched view calls (szhip_*_omp_batch_view): the number of gather / scatter launches of the call, 0 or 1 whatever `count` is */
    int book_on_device;     /* 1: the Huffman code book of this stream was built on the device (SZ_HIP_DEV_BOOK=1, szh_book.h); 0: on the host */
} szhip_stats;

int  szhip_create(szhip_ctx **ctx, int device);
/* ---- several arrays in flight on one GPU (additive; the reference's API is one blocking call per array, sz/src/sz.c:294-391).
 * The predict+quantise sweep is bound by its dependency chain, not by the chip: the passes in front of it (fit, sampling) and
 * behind it (block ordering, histogram, Huffman packing) of one array fit beside the sweep of another.  A pool owns `lanes`
 * contexts and as many host threads; szhip_pool_submit queues one szhip_compress call (same arguments, which must stay valid
 * until the wait returns) and returns a ticket at once; szhip_pool_wait blocks until that call has finished and hands out what
 * szhip_compress would have returned.  Streams are byte for byte those of szhip_compress.  HDF5 chunks (one SZ call per chunk,
 * hdf5-filter/H5Z-SZ/src/H5Z_SZ.c:542-828) and time steps are the natural users. */
typedef struct szhip_pool szhip_pool;
int  szhip_pool_create(szhip_pool **pool, int device, int lanes);
void szhip_pool_destroy(szhip_pool *pool);
int  szhip_pool_submit(szhip_pool *pool, int dtype, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, double eb,
                       const szhip_params *params, const unsigned char *meta, size_t meta_len, int out_on_device,
                       unsigned char *out_buf, size_t out_cap, int *ticket);      /* out_on_device 2: into out_buf (capacity out_cap) */
int  szhip_pool_wait(szhip_pool *pool, int ticket, unsigned char **out, size_t *out_size, szhip_stats *stats);   /* the call's return code */

void szhip_destroy(szhip_ctx *ctx);
const char *szhip_last_error(szhip_ctx *ctx);

/* copy a host array into the context's device input buffer once, so that szhip_minmax and
 * szhip_compress can both run on it (data_on_device = 1) without a second PCIe transfer */
int szhip_stage_input(szhip_ctx *ctx, const void *host_data, size_t bytes, void **device_ptr);
/* ... and `count` host arrays of `bytes` bytes each, one behind the other at multiples of 16 (one copy when they total at most 64 MiB): device_ptrs[i] then serves
 * as array i with data_on_device = 1 for szhip_minmax_batch and szhip_compress_omp_batch, so that a host array crosses the bus once for both */
int szhip_stage_input_batch(szhip_ctx *ctx, const void *const *host_data, int count, size_t bytes, const void **device_ptrs);
/* ... of different lengths, array i of bytes[i] bytes (for szhip_minmax_batch_lens and szhip_compress_omp_batch_shapes) */
int szhip_stage_input_batch_lens(szhip_ctx *ctx, const void *const *host_data, int count, const size_t *bytes, const void **device_ptrs);

/*
 * Device pointers and ordering (all calls below): a call runs on the context's own NON-BLOCKING streams and returns when its results are complete.
 * What it reads from device memory must be complete when the call is made: synchronise the stream that produces it first -- the null stream's
 * implicit ordering does not reach non-blocking streams, and a device-to-device hipMemcpy may return to the host before the copy has finished
 * (profiles/r06_device_input_ordering.txt: a tool that decoded a stream right behind such a copy read a stream whose end had not arrived).
 * Alignment: a pointer to VALUES -- `data` of szhip_minmax, of every compress call and of the prepare calls, `out` of every decompress call, d_src / d_out / d_data of
 * szhip_store_be / szhip_load_be / szhip_fill / szhip_clamp -- is aligned to its
 * element (4 bytes for SZHIP_F32, 8 for SZHIP_F64), on the host or on the device; any other address is refused with SZHIP_ERR_ARG before anything is launched or
 * written.  More is never required: an array that starts at any element of a larger allocation (a chunk of a buffer, a view that skips a row) is taken, and the
 * library itself picks the kernels that need 16-byte rows only where the address allows them -- same stream, same values.  BYTE pointers -- `stream`, `meta`, a
 * caller's stream buffer (out_on_device = 2), the output arrays of szhip_huff_book, `dst` of
 * szhip_store_be and `src` of szhip_load_be -- take any alignment.  Nothing is written in front of an output or behind
 * its end (r0*r1*r2 values of a decompress call, the capacity of a caller's stream buffer), and an input array is never written.
 * A caller's stream buffer (out_on_device = 2 of szhip_compress / szhip_pool_submit) is written IN PLACE exactly when its address is a multiple of 16 and its
 * capacity is at least the stream's length + 64 (with SZ_HIP_DEV_BOOK=1, where the length is not known before the kernels run: at least the header without the
 * tree + 18424 + 64 bytes, and a stream that leaves less than 64 bytes of the capacity free goes round again with the host's book); then bytes behind the stream,
 * up to the capacity, may be zeroed.  Otherwise the stream is built in the context's buffer and copied: then exactly its bytes are written.  A capacity below the
 * stream's length is SZHIP_ERR_ARG -- found when the length is known, at the end of the call; nothing outside the buffer has been written and the context stays usable.
 */
/* min / max of n values (device or host pointer) */
int szhip_minmax(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t n, double *vmin, double *vmax);
/*
 * ... of `count` arrays of n values each in ONE launch and ONE read-back of `count` pairs (kernel: sz_amd/csrc/szh_rangebatch.h): what a
 * range-based error bound needs before a batch compress call.  The array is the grid's second dimension; its base pointer comes through a device table that is
 * uploaded once.  Each array is contiguous and aligned to its element, and is cut at the 16-byte boundaries of its OWN address: the pieces between move 16 bytes per
 * lane, the head and the tail value by value -- so the arrays of a batch may lie at different offsets from a boundary.
 * vmin[i] / vmax[i] are bit for bit what szhip_minmax returns for array i alone: a NaN takes no part, zeros of both signs are ordered -0.0 < +0.0, an array
 * without a number gives what szhip_minmax gives (min and max do not depend on the order of reduction; the reduction is over ordered integers, no float atomics).
 * Host arrays (data_on_device = 0) are staged one behind the other into the context's input buffer, as szhip_compress_omp_batch stages them.
 * SZHIP_ERR_ARG before anything is launched: count < 1, n == 0, a null pointer, a pointer that is not aligned to its element.  SZHIP_ERR_UNSUP beyond
 * count <= 65535 and count x n < 2^32, the limits of the batch.  stats (may be NULL): quant_kernel_launches is the number of scan launches, 1 whatever `count` is.
 */
int szhip_minmax_batch(szhip_ctx *ctx, int dtype, const void *const *data, int count, int data_on_device, size_t n, double *vmin, double *vmax,
                       szhip_stats *stats);
/*
 * ... of `count` SUB-BOXES of r0 x r1 x r2 values with the common element pitches pitch0 / pitch1 (the VIEWS below; data[i] is sub-box i's first value), still one
 * launch and one read-back: every ROW is cut at its own 16-byte boundaries as the call above cuts every array (k_minmax_batch_view: a group of lanes per row), so
 * vmin[i] / vmax[i] are bit for bit szhip_minmax of a contiguous copy of sub-box i, and nothing outside the sub-boxes is read.  pitch1 == r2 with pitch0 == r1 * r2 is
 * the call above, exactly.  Sub-boxes on the host: their rows alone are staged, packed.  Arguments and limits as above, on r0 x r1 x r2 values; pitch1 < r2 or
 * pitch0 < r1 * pitch1: SZHIP_ERR_ARG.
 */
int szhip_minmax_batch_view(szhip_ctx *ctx, int dtype, const void *const *data, int count, int data_on_device, size_t r0, size_t r1, size_t r2,
                            size_t pitch0, size_t pitch1, double *vmin, double *vmax, szhip_stats *stats);

/*
 * Compress a 3-D array (r0 slowest ... r2 fastest, the callee convention of sz_float.c:6527) with
 * absolute bound `eb` (already derived from the user's mode by the caller, sz_float.c:2852-2868).
 * r0 == 0: a 2-D array r1 x r2 (SZ_compress_float_2D_MDQ_nonblocked_with_blocked_regression, sz_float.c:5516 /
 * sz_double.c:4900): 16-wide blocks, three plane coefficients per block.
 * `meta`/`meta_len`: the 3 version bytes + flag byte + parameter bytes the stream starts with.
 * Output: out_on_device = 0: *out is malloc'd host memory owned by the caller (free());
 *         out_on_device = 1: *out is a device pointer owned by ctx (valid until the next call);
 *         out_on_device = 2: *out is the CALLER's device buffer of capacity *out_size; the stream is written there -- in place when the buffer is
 *                            16-byte aligned and holds the stream plus 64 bytes of slack (bytes behind the stream, up to the capacity, may be
 *                            zeroed), else through the context's buffer and a copy.
 */
int szhip_compress(szhip_ctx *ctx, int dtype, const void *data, int data_on_device,
                   size_t r0, size_t r1, size_t r2, double eb, const szhip_params *params,
                   const unsigned char *meta, size_t meta_len,
                   int out_on_device, unsigned char **out, size_t *out_size, szhip_stats *stats);

/*
 * Decompress a SZ 2.1 regression-type stream.  `stream` points at the first byte of the whole stream
 * (version bytes); `body_off` is the offset of the block-size field (4 + 28|36 + 8).
 * `out`: device pointer (out_on_device) or host pointer to r0*r1*r2 values.  r0 == 0: a 2-D array r1 x r2
 * (decompressDataSeries_float_2D_nonblocked_with_blocked_regression, szd_float.c:3141 / szd_double.c:2974).
 */
int szhip_decompress(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len,
                     size_t body_off, size_t r0, size_t r1, size_t r2,
                     void *out, int out_on_device, szhip_stats *stats);

/*
 * SZ 1.4 ("withLinearRegression = NO") path for 3-D arrays: whole-array Lorenzo prediction with lossy "exact" values and the
 * TightDataPointStorage container.  Replaces SZ_compress_float_3D_MDQ + convertTDPStoFlatBytes_float (sz/src/sz_float.c:946-1415,
 * TightDataPointStorageF.c:379-479,590-663; doubles: sz_double.c:784, TightDataPointStorageD.c) as called from
 * SZ_compress_args_float_NoCkRngeNoGzip_3D (sz_float.c:1422).  `value_range` and `median` are the range scan's results
 * (max - min and min + range/2 in the data's type, dataCompression.c:102-119); `meta` as for szhip_compress, with the flag byte of
 * TightDataPointStorageF.c:600-611.  r0 == 0: a 2-D array r1 x r2 (SZ_compress_float_2D_MDQ, sz_float.c:610-894, called from :896).
 * r0 == 0 and r1 == 0: a 1-D array of r2 values (SZ_compress_float_1D_MDQ, sz_float.c:353-540, called from :561; doubles:
 * sz_double.c:260); the caller applies the call site's own raw-store rule (sz_float.c:2908).
 */
int szhip_compress_sz14(szhip_ctx *ctx, int dtype, const void *data, int data_on_device,
                        size_t r0, size_t r1, size_t r2, double eb, double value_range, double median,
                        const szhip_params *params, const unsigned char *meta, size_t meta_len,
                        int out_on_device, unsigned char **out, size_t *out_size, szhip_stats *stats);
/* Inverse: decompressDataSeries_float_3D (sz/src/szd_float.c:600-1138; doubles: szd_double.c) on a TightDataPointStorage stream
 * (parse: TightDataPointStorageF.c:54-265).  `body_off` is the offset of the max_quant_intervals field (4 + 28|36 + 8).
 * r0 == 0: a 2-D array (decompressDataSeries_float_2D, szd_float.c:284-598); r0 == 0 and r1 == 0: a 1-D array
 * (decompressDataSeries_float_1D, szd_float.c:185-282). */
int szhip_decompress_sz14(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len,
                          size_t body_off, size_t r0, size_t r1, size_t r2, void *out, int out_on_device, szhip_stats *stats);

/*
 * The reference's OpenMP container for 3-D arrays -- replaces SZ_compress_float_3D_MDQ_openmp (sz/src/sz_omp.c:63-358; double :578-863; box
 * quantiser SZ_compress_float_3D_MDQ_RA_block, sz/src/sz_float.c:4704-5012) and decompressDataSeries_float_3D_openmp (sz_omp.c:366-566):
 * the array is cut into the box grid of `thread_num` (sz_omp.c:88-117; what an OpenMP build takes from omp_get_max_threads()), every box is
 * quantised on its own from its own reconstructed neighbours, one Huffman code book covers all boxes, every box has a byte-aligned payload.
 * A stock OpenMP build of SZ reads the stream; the box count is in it.  `meta`: the 4 + MetaDataByteLength bytes the reference writes in
 * front (version, flag byte, parameter bytes); `eb`: the absolute bound (`realPrecision`).  params->quantization_intervals == 0: the
 * interval optimiser of the SZ 1.4 path over the whole array (optimize_intervals_float_3D_opt, sz_omp.c:73-82).
 * Restrictions (SZHIP_ERR_UNSUP otherwise): the box grid must divide the array (on an uneven grid the reference's code book depends on
 * uninitialised memory), a box face (dim 0 x dim 1 of a box) has at most 1024 rows -- thread_num 4096 cuts 512^3 into 32^3 boxes.
 * `body_off` of the inverse: offset of the thread_num field (4 + MetaDataByteLength).
 * Status (round 4): on MI355X byte-identical to the oracle (oracle/szo_omp_impl.h) and md5-identical to 12 recorded outputs of the reference built
 * with -fopenmp (8 float32; 4 float64 from the same sources at -O1).  Boxes with 32 x 32 faces run the column-per-lane sweep of szh_ompcol.h
 * (k_omp_col: 0.16 ms at 512^3 f32, the whole call 0.69 ms = 777 GB/s); other shapes the first form (k_omp_box).
 */
int szhip_compress_omp(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, double eb,
                       int thread_num, const szhip_params *params, const unsigned char *meta, size_t meta_len,
                       int out_on_device, unsigned char **out, size_t *out_size, szhip_stats *stats);
int szhip_decompress_omp(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len,
                         size_t body_off, size_t r0, size_t r1, size_t r2, void *out, int out_on_device, szhip_stats *stats);
/*
 * A sub-box of an OpenMP-container stream: `out` (host or device, as above) receives the (hi[0]-lo[0]) x (hi[1]-lo[1]) x (hi[2]-lo[2]) values of
 * [lo, hi) -- dim 0 slowest, `hi` exclusive --, contiguous, bit for bit the crop of what szhip_decompress_omp writes for the same stream; no byte
 * outside that buffer is written.  Only the boxes that meet the region are decoded (every box restarts the predictor and has its own payload):
 * device work, copies and workspace grow with their number, the host walks the stream's per-box tables once.  Of a host stream the tables and the
 * spans of the covered boxes are uploaded, not the stream.  A region that ends on box boundaries is written by the sweeps themselves; any other goes
 * through a staging array of the covered boxes and is cropped out of it (k_omp_crop).
 * stats: n_blocks the boxes decoded, n_elements the region's values, n_unpred the verbatim values of the decoded boxes; quant_kernel as above.
 * NOT validated: boxes the region does not touch.  The header and table checks of szhip_decompress_omp are made (SZHIP_ERR_STREAM / SZHIP_ERR_UNSUP
 * exactly where it gives them), the payloads and verbatim-value counts are checked for the decoded boxes only -- a damaged payload elsewhere is
 * neither detected nor does it affect the result.  SZHIP_ERR_ARG: lo[d] >= hi[d], or hi[d] beyond the extent.
 */
int szhip_decompress_omp_region(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len,
                                size_t body_off, size_t r0, size_t r1, size_t r2, const size_t lo[3], const size_t hi[3],
                                void *out, int out_on_device, szhip_stats *stats);

/*
 * VIEWS: a sub-box of a larger array, compressed from and decoded into where it lies.  A view is r0 x r1 x r2 values (dim 0 slowest), given by a pointer to its
 * first value and two ELEMENT pitches: pitch0 between successive dim-0 planes, pitch1 between successive dim-1 rows; pitch1 >= r2 and pitch0 >= r1 * pitch1 (pitch0
 * need not be a multiple of pitch1), anything else is SZHIP_ERR_ARG before anything is launched or written.  pitch1 == r2 and pitch0 == r1 * r2 is the contiguous
 * array.  The bar: a stream made from a view is byte for byte the stream the same call makes from a contiguous copy of the sub-box; decoding into a view writes bit for
 * bit what the contiguous decode writes, into the sub-box and nowhere else -- not between rows, not between planes, not in front or behind; an input view is never
 * written.  Alignment: the base pointer to its element, as everywhere; the restrictions and error codes of the contiguous calls apply to the sub-box's extents.
 *
 * szhip_compress_omp_view / szhip_decompress_omp_view: the OpenMP container, DIRECTLY on a device view -- no packing pass, no staging array: the sweeps, the encoders'
 * reads of verbatim values and the inverse sweeps address the parent array through the pitches, and the interval optimiser (params->quantization_intervals == 0)
 * samples the points it samples on the contiguous copy (the lattice is the sub-box's, only the addresses take the pitches: k_sample_view).  The 16-byte forms
 * (stats.quant_kernel 3 and 4) need the base address, pitch1 and pitch0 to be multiples of 16 bytes.  A view that misses them while its boxes have 32 x 32 faces (the
 * column form's shape; e.g. float32 with 1 - 3 ghost values) is packed into (decoded in) the context's contiguous buffer by the call itself and runs the column form
 * there -- value by value it took 4.3 x / 2.7 x as long --; stats.quant_kernel reports 3.  Any other view that misses them takes the value-by-value form (5) where it
 * lies.  The stream is the same in every case.  A view on the HOST (data_on_device = 0 / out_on_device = 0): only the sub-box's rows cross the bus, into or out of the context's contiguous buffer
 * (the host's copy into the pinned staging buffers walks the rows); then the contiguous call runs, and of a damaged stream nothing reaches the caller's array.
 *
 * szhip_pack_view / szhip_scatter_view serve every other stream type at the cost of ONE pass over the sub-box: the strided reads are NOT inside k_beam, k_pencil,
 * k_fit_select or the SZ 1.4 sweeps (their geometry also places the codes).  szhip_pack_view gathers the view (device or host) into the context's input buffer, as
 * szhip_stage_input does with a contiguous host array: *d_packed then serves as `data` with data_on_device = 1 for szhip_minmax, szhip_compress,
 * szhip_compress_sz14 and the PW_REL prepare calls (valid until the next call that stages an input).  szhip_scatter_view puts a decoded contiguous DEVICE array
 * (r0 x r1 x r2 values at d_packed) into a view on the device (k_view_scatter: rows move 16 bytes per lane between the 16-byte boundaries of the destination, a
 * value-by-value head and tail per row, no read of the view) or on the host.  Both take 2-D views as r0 == 0 (pitch0 is ignored).
 * Costs (MI355X, 512^3 float32, device-resident): the direct calls on an aligned view 1.04 x / 1.03 x the contiguous calls and 0.85 x / 0.83 x pack + compress /
 * decompress + scatter; packing 0.15 ms, scattering 0.24 ms; SZ 2.1 from a view 1.11 x the contiguous call.
 * Many views of one shape in one call: szhip_compress_omp_batch_view / szhip_decompress_omp_batch_view, szhip_minmax_batch_view, szhip_compare_batch_view (below).
 * Sub-boxes of many streams into views in one call: szhip_decompress_omp_batch_region (below; count 1 is region decode into a view).
 * Not covered: a strided single-array szhip_minmax (szhip_minmax_batch_view with count 1 serves), the slab container.
 */
int szhip_compress_omp_view(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1,
                            double eb, int thread_num, const szhip_params *params, const unsigned char *meta, size_t meta_len,
                            int out_on_device, unsigned char **out, size_t *out_size, szhip_stats *stats);
int szhip_decompress_omp_view(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len,
                              size_t body_off, size_t r0, size_t r1, size_t r2, void *out, int out_on_device, size_t pitch0, size_t pitch1, szhip_stats *stats);
int szhip_pack_view(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t r0, size_t r1, size_t r2, size_t pitch0, size_t pitch1, void **d_packed);
int szhip_scatter_view(szhip_ctx *ctx, int dtype, const void *d_packed, size_t r0, size_t r1, size_t r2, void *out, int out_on_device, size_t pitch0, size_t pitch1);

/*
 * MANY SMALL ARRAYS of one shape in one call (OpenMP container).  A single call's cost for a small array is almost entirely fixed -- host
 * synchronisations, launch gaps, small copies, kernels that cannot fill the chip with 8 - 27 boxes.  A batch call runs the container's kernels ONCE over the boxes of all
 * `count` arrays (the array is the grid's second dimension; a box finds its array's base pointer, bound, interval count, code table and stream position through a
 * per-array table), builds `count` code books on the host between two synchronisations, and so makes a number of synchronisations, launches and copies that does not
 * grow with `count` (one sweep launch per form, below).  The shape r0 x r1 x r2, dtype, thread_num, params, meta_len and the pointer kinds are common; everything else
 * is per item.  No stream changes:
 *   - blob[offset_i, offset_i + size_i) is byte for byte what szhip_compress_omp returns for array i alone with the same eb, meta, params and thread_num; the
 *     interval optimiser (params->quantization_intervals == 0) runs per array, so the arrays of a batch may have different interval counts, trees and header lengths.
 *     Offsets increase with i and are multiples of 64; bytes between streams are undefined.  *blob: out_on_device 0: malloc'd host memory owned by the caller (free());
 *     1: device memory owned by the context (valid until its next batch compress call); 2 (a caller's buffer): SZHIP_ERR_UNSUP.
 *   - the batched decode writes into items[i].out bit for bit what szhip_decompress_omp writes for stream i, and nothing else.  Inputs are never written.
 * Alignment as above: values to their element, streams and meta any; the 16-byte forms are picked PER ARRAY from its address, so the arrays of a batch may take
 * different sweep forms (items[i].quant_kernel 3 / 4 / 5): they are grouped by form, one sweep launch per form; stats->quant_kernel_launches counts the sweep launches
 * of the shared part (at most 3; the single calls of fallback items are not in it).
 * Fallback: an array the shared launches do not cover runs through the single call from inside the batch call (identical by construction), its stream goes into the
 * blob / its values into `out`, items[i].batched = 0, the rest of the batch stays batched.  Compress: more than 1024 intervals, a longest code word above 32 bits, a box
 * of a number of points that is no multiple of 8 (then the whole batch), an extent of 1 in dim 0 or dim 1 (the whole batch).  Decompress: a one-symbol book, a stream
 * that misses the look-up-table decoder's conditions (box points no multiple of 8; payload + tables beyond a workgroup's LDS), a thread_num other than the batch's first.
 * Errors: the call returns the first non-zero items[i].rc, else SZHIP_OK.  A decompress item that fails (SZHIP_ERR_STREAM: found on the host in its header and tables,
 * or on the device in its payloads and verbatim-value counts, counted per array) does not disturb the others: items with rc == SZHIP_OK are fully and correctly decoded, a
 * failed item's output array is undefined.  Refused with SZHIP_ERR_ARG before anything is launched or written: count < 1, a null item pointer (data / meta; stream /
 * out), a misaligned value pointer, a bound that is not positive.
 * Limits (SZHIP_ERR_UNSUP beyond them): count <= 65535, count x boxes <= 2^22, count x r0 x r1 x r2 < 2^32 values; the single call's restrictions on the shape.
 * Host arrays (data_on_device = 0) are staged one behind the other into the context's input buffer with ONE copy when they total at most 64 MiB, else array by array.
 * stats: n_elements / n_blocks / n_unpred / out_bytes are sums over the batch, the times those of the shared launches.
 */
typedef struct szhip_batch_item {
    /* in  */ const void *data;             /* compress: the array; decompress: unused */
              void *out;                    /* decompress: where the array goes */
              double eb;                    /* compress: absolute bound of THIS array */
              const unsigned char *meta;    /* compress: meta_len bytes in front of THIS stream */
              const unsigned char *stream;  /* decompress: the stream's first byte ... */
              size_t stream_len, body_off;  /* ... its length, the offset of its thread_num field */
    /* out */ size_t offset, size;          /* compress: the stream's place in the blob */
              int rc;                       /* SZHIP_* of this item */
              unsigned intervals;
              uint64_t n_unpred;
              int quant_kernel;             /* 3 / 4 / 5 as in szhip_stats */
              int batched;                  /* 1: ran in the shared launches; 0: the single call ran for it */
} szhip_batch_item;
int szhip_compress_omp_batch(szhip_ctx *ctx, int dtype, szhip_batch_item *items, int count, int data_on_device, size_t r0, size_t r1, size_t r2, int thread_num,
                             const szhip_params *params, size_t meta_len, int out_on_device, unsigned char **blob, size_t *blob_size, szhip_stats *stats);
int szhip_decompress_omp_batch(szhip_ctx *ctx, int dtype, szhip_batch_item *items, int count, int stream_on_device, size_t r0, size_t r1, size_t r2,
                               int out_on_device, szhip_stats *stats);
/*
 * BATCHES OF VIEWS: many same-shape PATCHES WITH GHOST LAYERS in one call -- the interiors of the padded arrays of a block-structured code.
 * The batch calls above on sub-boxes: r0 x r1 x r2, dtype, thread_num, params, meta_len, the pointer kinds AND the two element pitches (the meaning and the rules of
 * the VIEWS above: pitch1 >= r2, pitch0 >= r1 * pitch1, pitch0 need not be a multiple of pitch1; anything else SZHIP_ERR_ARG before anything is launched or written)
 * are common; items[i].data / items[i].out is the FIRST VALUE of sub-box i.  pitch1 == r2 with pitch0 == r1 * r2 is the contiguous batch call, exactly.
 * The bar is the union of the two bars: blob[offset_i, offset_i + size_i) is byte for byte what szhip_compress_omp makes from a contiguous copy of sub-box i; the
 * batched decode writes into sub-box i bit for bit what szhip_decompress_omp writes, and no other byte of any parent -- not between rows, not between planes, not in
 * the ghost layers, not in front or behind; inputs are never written.
 * Form PER ITEM, from its own base address and the common pitches (items[i].quant_kernel):
 *   - base, pitch1 and pitch0 all multiples of 16 bytes: the column form (3) or the vector box form (4) DIRECTLY on the parent, through the pitches;
 *   - any of them off, boxes with 32 x 32 faces (e.g. float32 with 1 - 3 ghost values): the view is GATHERED into (decoded in) a contiguous copy in the context's
 *     input (output) buffer and runs the column form there; quant_kernel reports 3, as the single view call does.  ONE gather launch (k_ompb_crop) covers all such
 *     items of a compress call, ONE scatter launch (k_ompb_view_scatter: 16 bytes per lane between the 16-byte boundaries of each destination row, a value-by-value
 *     head and tail, no read of the view) all such items of a decode that decoded without error -- of a damaged stream nothing reaches its parent;
 *   - any other view that misses the 16 bytes: the value-by-value form (5) where it lies.
 * stats->quant_kernel_launches: one sweep launch per form AND addressing (direct / gathered) that occurs in the batch -- at most 2 (the column shape: 3 direct and 3
 * gathered; any other shape: 4 and 5); stats->packing: the gather / scatter launches of the call, counted where they are launched: 0 or 1.  Neither grows with `count`, nor do the synchronisations and copies.
 * The interval optimiser samples every view where it lies (k_ompb_sample_view: the lattice of the contiguous copy, addresses through the pitches).
 * Fallbacks, errors and limits are those of the contiguous batch calls on the sub-box's extents; a fallback item runs szhip_compress_omp_view /
 * szhip_decompress_omp_view from inside the call (items[i].batched = 0).  Views on the HOST (data_on_device / out_on_device = 0): only the sub-boxes' rows cross the
 * bus, staged one behind the other; then the contiguous batch runs, and of a damaged stream nothing reaches the caller's parent.  out_on_device = 2 of the compress
 * call stays SZHIP_ERR_UNSUP.  A device view inside the context's input buffer (what szhip_stage_input handed out) is SZHIP_ERR_ARG before anything is launched: the gather uses that buffer.
 * Cost (MI355X, 64 patches of 64^3 float32, device-resident): DESIGN section 4.5.6.
 */
int szhip_compress_omp_batch_view(szhip_ctx *ctx, int dtype, szhip_batch_item *items, int count, int data_on_device, size_t r0, size_t r1, size_t r2,
                                  size_t pitch0, size_t pitch1, int thread_num, const szhip_params *params, size_t meta_len, int out_on_device,
                                  unsigned char **blob, size_t *blob_size, szhip_stats *stats);
int szhip_decompress_omp_batch_view(szhip_ctx *ctx, int dtype, szhip_batch_item *items, int count, int stream_on_device, size_t r0, size_t r1, size_t r2,
                                    int out_on_device, size_t pitch0, size_t pitch1, szhip_stats *stats);
/*
 * ARRAYS OF DIFFERENT SHAPES in one call: the patches of an AMR level, inner and edge chunks of a dataset, the tensors of a checkpoint.  The
 * batch calls above with the shape AND thread_num per item: item i is a contiguous array of shapes[i].r0 x r1 x r2 values (dim 0 slowest) cut into
 * shapes[i].thread_num boxes.  dtype, params, meta_len and the pointer kinds stay common.  The bar is the same-shape call's, per item:
 *   - blob[offset_i, offset_i + size_i) is byte for byte what szhip_compress_omp returns for array i alone with shapes[i], items[i].eb, items[i].meta and params;
 *     offsets are multiples of 64 and increase with i; out_on_device = 2 stays SZHIP_ERR_UNSUP;
 *   - the batched decode writes into items[i].out bit for bit what szhip_decompress_omp writes for stream i, and nothing else; inputs are never written.  The box
 *     count is read from each stream (shapes[i].thread_num is ignored); a stream is batched when the grid of ITS thread_num divides ITS shape -- the same-shape
 *     call's "thread_num of the batch's first stream" rule does not exist here --, anything else goes to the single call, which says what is wrong with it.
 * Launches, synchronisations and copies do not grow with `count`, only with the number of KINDS of item: every item's geometry (box grid, sampler lattice and row
 * limit, boxes per histogram workgroup, flag words) is computed on the host and reaches the kernels through a second per-item record; the first dimension of every
 * launch is sized to its largest item and the surplus workgroups of the smaller ones return at once.  The column form (3) takes every item with 32 x 32 box faces in
 * ONE launch, whatever its plane count and box count; the box forms (4, 5) take one launch per distinct box c0 x c1 x c2, because the block is the box's face and
 * the LDS its ring.  stats->quant_kernel_launches is therefore at most the number of distinct (form, c0 x c1 x c2) among the batched items, and is the same when
 * every item is given twice.  One sampling launch, one histogram read-back, `count` host books between two synchronisations, one encode phase, as above.  A kind with
 * a single member still runs in the shared launches.
 * Work arrays (codes, per-box counts, first values, sizes, offsets, ranks, histograms, verbatim values, flag words, the decoder's staging) lie one item behind the
 * other at each item's own length, each at the alignment the single call gives it.  Host arrays are staged one behind the other at their own lengths.
 * Fallbacks are PER ITEM (items[i].batched = 0; the rest stays batched): boxes of a number of points that is no multiple of 8, an extent of 1 in dim 0 or dim 1, and
 * those of the same-shape call (more than 1024 intervals, a code word above 32 bits; decode: a one-symbol book, a stream beyond the look-up-table decoder's LDS).
 * Errors: per-item rc as above.  An item whose shape the single call refuses (no dividing grid, a box face above 1024 rows) gets that rc and an empty stream; the rest
 * proceed.  SZHIP_ERR_ARG before anything is launched or written: count < 1, null `shapes`, an extent of 0 or above 2^31 - 1, thread_num < 1 (compress), and the
 * same-shape call's refusals.  SZHIP_ERR_UNSUP beyond: count <= 65535, boxes of all items <= 2^22, values of all items < 2^32.
 * Not covered: compress from / full decode into views with per-item pitches (sub-boxes of streams into such views: szhip_decompress_omp_batch_region), mixed dtypes, items that are not 3-D, szhip_compare_batch on pairs of different lengths (it is element-wise: group by length).
 */
typedef struct szhip_batch_shape { size_t r0, r1, r2; int thread_num; } szhip_batch_shape;
int szhip_compress_omp_batch_shapes(szhip_ctx *ctx, int dtype, szhip_batch_item *items, const szhip_batch_shape *shapes, int count, int data_on_device,
                                    const szhip_params *params, size_t meta_len, int out_on_device, unsigned char **blob, size_t *blob_size, szhip_stats *stats);
int szhip_decompress_omp_batch_shapes(szhip_ctx *ctx, int dtype, szhip_batch_item *items, const szhip_batch_shape *shapes, int count, int stream_on_device,
                                      int out_on_device, szhip_stats *stats);
/* szhip_minmax_batch with a length per array (lens[i] >= 1 values): bit for bit szhip_minmax of each array (ordered-integer reduction, a NaN takes no part), ONE launch
 * whose grid is sized to the longest array (the surplus workgroups of a shorter one return), one read-back.  An element-aligned base at any offset from a 16-byte
 * boundary is accepted.  Limits: count <= 65535, fewer than 2^32 values in all. */
int szhip_minmax_batch_lens(szhip_ctx *ctx, int dtype, const void *const *data, const size_t *lens, int count, int data_on_device, double *vmin, double *vmax,
                            szhip_stats *stats);
/*
 * SUB-BOXES OF MANY STREAMS in one call: the faces of neighbouring patches that fill ghost layers, slices through a level, the boxes a probe
 * touches.  szhip_decompress_omp_region per item, with the per-call costs of szhip_decompress_omp_batch_shapes: item i names an OpenMP-container stream (items[i].stream,
 * stream_len, body_off) of an array of shapes[i].r0 x r1 x r2 values -- the box count is read from the stream, shapes[i].thread_num is ignored --, the sub-box
 * [regions[i].lo, regions[i].hi) of it (dim 0 slowest, hi exclusive) and a destination items[i].out (host or device, aligned to its element) with the two ELEMENT
 * pitches of the VIEWS above (pitch1 >= hi[2] - lo[2], pitch0 >= (hi[1] - lo[1]) * pitch1, pitch0 need not be a multiple of pitch1; 0, 0: contiguous).
 * The bar: the destination sub-box receives bit for bit the crop [lo, hi) of what szhip_decompress_omp writes for that stream -- NaN payloads and signed zeros
 * included; what szhip_decompress_omp_region returns --, and NO other byte of any destination allocation is written: not between rows or planes, not in front or
 * behind, not in ghost cells outside the sub-box.  Destinations are never read, streams never written.  Destinations of different items that overlap: undefined.
 * Work: launches, synchronisations and copies grow with the number of KINDS of item, not with `count`.  Every item's "array" is the sub-array of the boxes its region
 * meets: compact tables in sub-grid order and a sub-geometry per item, the k_ompbs_* launches of the different-shapes call over them.  The covered boxes' first values,
 * verbatim values and payloads are fetched by ONE gather launch over all items' spans (device streams) or go up as ONE pinned blob (host streams); whole streams are
 * not copied, and only header prefixes and tables reach the host.  Every item is swept into a staging array in the context -- form per item by the single region call's
 * rule on the sub-geometry: the column form (3) needs 32 x 32 faces and an even covered-box count, anything else a box form (4 / 5); one sweep launch per distinct
 * (form, box c0 x c1 x c2) --, and ONE placing launch (k_ompbr_place; stats->packing = 1) puts every region into its destination: 16 bytes per lane between the
 * 16-byte boundaries of each destination row, a value-by-value head and tail, no read of the destination.  The placing launch reads the sweeps' error counts on the
 * device: no synchronisation lies in front of it, and an item that fails leaves its destination untouched.  A host destination is placed contiguous into a device buffer
 * by the same launch and its rows are copied out through the pitches; of a failed item nothing is copied.
 * Items with the same (stream, stream_len, body_off) and shape share one header read, one table walk, one tree, one node table and one look-up-table build;
 * regions[i].shares is the first such item.  Host header work and header fetches grow with the number of DISTINCT streams.
 * Fallbacks PER ITEM (items[i].batched = 0, the rest stays batched; szhip_decompress_omp_region from inside the call, a view placed behind it): a one-symbol book, box
 * points that are no multiple of 8, covered payloads plus tables beyond a workgroup's LDS, a stream whose grid does not divide its shape (the single call says what is
 * wrong with it).
 * Errors: per-item rc, the call returns the first non-zero one.  SZHIP_ERR_STREAM is found on the host in headers and tables and on the device in the payloads and
 * verbatim-value counts of COVERED boxes only; boxes no region touches are not validated.  A failed item disturbs no other item -- not another region of the same
 * stream whose boxes are sound.  SZHIP_ERR_ARG before anything is launched or written: count < 1; null shapes, regions, stream or out; a misaligned out; lo[d] >= hi[d]
 * or hi[d] beyond the extent; pitches that break the view rule.  SZHIP_ERR_UNSUP beyond: count <= 65535, covered boxes of all items <= 2^22, staged values (covered
 * boxes x box points) of all items < 2^32.
 * stats: n_elements the values delivered, n_blocks the boxes decoded, n_unpred their verbatim values (the sums of what szhip_decompress_omp_region reports per item);
 * quant_kernel_launches the sweep launches, packing the placing launches (0 or 1); items[i].quant_kernel / intervals / n_unpred per item.
 * Not covered: a direct form (the sweeps writing straight into a destination whose region ends on box boundaries -- every item goes through the staging array), a dtype per item.
 */
typedef struct szhip_batch_region {
    /* in  */ size_t lo[3], hi[3];      /* the sub-box of THIS item's array, dim 0 slowest, hi exclusive */
              size_t pitch0, pitch1;    /* element pitches of the destination; 0, 0: contiguous (hi-lo extents) */
    /* out */ uint64_t n_boxes;         /* boxes decoded for this item */
              int shares;               /* index of the first item that names the same stream (i itself otherwise) */
} szhip_batch_region;
int szhip_decompress_omp_batch_region(szhip_ctx *ctx, int dtype, szhip_batch_item *items, const szhip_batch_shape *shapes, szhip_batch_region *regions, int count,
                                      int stream_on_device, int out_on_device, szhip_stats *stats);

/*
 * Point-wise relative bounds (PW_REL and its AND/OR combinations) in their log-domain form: the `_pwr_pre_log` functions of
 * sz/src/sz_float_pwr.c:1791-1975 / sz_double_pwr.c:1781-1965 (dispatch sz_float.c:2888-2996) and their inverses
 * szd_float_pwr.c:1353-1422.  Three steps, the sign bytes being compressed on the host (zstd) in between:
 *   szhip_pwr_prepare       log2|x| into a device array owned by the context (*d_log), sign bytes to `signs_host` (n bytes) when any
 *                           value is negative (*positive == 0), and what the quantiser needs: the absolute bound in the log domain
 *                           (*real_precision), the log array's range and median, and the header's minLogValue.
 *                           vmin / vmax: the array's range (szhip_minmax).
 *   szhip_compress_sz14_pwr szhip_compress_sz14 on that array, writing the extra PW_REL container fields (TightDataPointStorageF.c:
 *                           408-419, 454-467): radExpo, segment_size, the compressed sign bytes and minLogValue.
 *   szhip_sz14_pwr_locate   (host only) where a PW_REL stream keeps its sign bytes, and its minLogValue;
 *   szhip_decompress_sz14_pwr  the SZ 1.4 inverse on a stream with those fields, then x = exp2(l) (0 below minLogValue), signs applied
 *                           (`signs_host`: n bytes or NULL).  Of a device-resident stream only the fixed fields in front of the type array come to the host.
 * The reference's DEFAULT form of mode PW_REL (accelerate_pw_rel_compression = 1, ratio >= 1e-5: the table-driven "MSST19" quantiser,
 * sz_float.c:1824-2725, dispatch :2838, :2890; inverse szd_float.c:1702-2700, szd_float_pwr.c:1425-1528; stream flag 0x08):
 *   szhip_msst_prepare      the scan of computeRangeSize_float_MSST19 (dataCompression.c:121-166: sign bytes from element 1 on, nearZero) and
 *                           a device copy of the array with its zeros replaced by nearZero * (1+ratio)^-3.0001 (*d_prepared, owned by the
 *                           context); the header's median (sqrt|nearZero * vmax|) and minLogValue (nearZero / (1+ratio)^2).
 *   szhip_compress_sz14_pwr with pwr->msst19 = 1, `eb` = the ratio and `data` = *d_prepared: multiplicative Lorenzo predictor on the
 *                           reconstruction, codes from the look-up table of MultiLevelCacheTableWideInterval.c:53-107 (built on the host).
 *   szhip_decompress_sz14_pwr  recognises the form by the stream's flag byte.
 * 2-D and 3-D arrays run on the wavefront kernel (szh_pencil.h, fmt 2); SZ_HIP_MSST_SWEEP=1 selects the plane-by-plane sweep of szh_msst.h
 * instead (second mapping, same bits); 1-D arrays are a one-lane chain.
 */
typedef struct szhip_pwr {
    uint64_t segment_size;             /* confparams_cpr->segment_size, recorded in the header */
    const unsigned char *signs_blob;   /* compressed sign bytes (host memory) or NULL */
    uint32_t signs_blob_size;
    double min_log_value;
    unsigned char rad_expo;            /* 0 on this path */
    unsigned char msst19;              /* 1: the table-driven form (below); `eb` of szhip_compress_sz14_pwr is then the ratio itself */
    unsigned char plus_bits;           /* confparams_cpr->plus_bits (3, conf.c:97), recorded in an MSST19 header */
    double median_stored;              /* MSST19: the header's median field, sqrt|nearZero * max| (sz_float_pwr.c:2060) */
} szhip_pwr;
int szhip_pwr_prepare(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t n, double vmin, double vmax, double pwr_ratio,
                      void **d_log, unsigned char *signs_host, int *positive, double *real_precision, double *value_range, double *median,
                      double *min_log_value);
int szhip_msst_prepare(szhip_ctx *ctx, int dtype, const void *data, int data_on_device, size_t n, double vmax, double pwr_ratio,
                       void **d_prepared, unsigned char *signs_host, int *positive, double *near_zero, double *median_log, double *min_log_value);
int szhip_compress_sz14_pwr(szhip_ctx *ctx, int dtype, const void *data, int data_on_device,
                            size_t r0, size_t r1, size_t r2, double eb, double value_range, double median,
                            const szhip_params *params, const unsigned char *meta, size_t meta_len, const szhip_pwr *pwr,
                            int out_on_device, unsigned char **out, size_t *out_size, szhip_stats *stats);
int szhip_sz14_pwr_locate(int dtype, const unsigned char *stream, size_t stream_len, size_t body_off, size_t *blob_off, size_t *blob_size,
                          double *min_log_value);
int szhip_decompress_sz14_pwr(szhip_ctx *ctx, int dtype, const unsigned char *stream, int stream_on_device, size_t stream_len,
                              size_t body_off, size_t r0, size_t r1, size_t r2, const unsigned char *signs_host, void *out,
                              int out_on_device, szhip_stats *stats);

/*
 * The Huffman code book of a code histogram, built on the device (k_huff_book, sz_amd/csrc/szh_book.h) -- what the reference's constructor and tree
 * serialiser do on the host (Huffman.c:76-185 build, :122-157 code words, :443-585 convert_HuffTree_to_bytes), bit for bit: same heap order among equal counts,
 * same node numbering, same node-index width.  szhip_compress uses the kernel when SZ_HIP_DEV_BOOK=1 is set; this entry runs it alone.
 * `hist`: `intervals` counts (1 .. 65536), a device or a host pointer.  Host outputs: `out_tree` (capacity out_tree_cap; record->tree_bytes are valid),
 * `out_code64` / `out_len8`: `intervals` right-aligned code words and their lengths (0 for a symbol that does not occur).
 * record->status != 0: the kernel declined and wrote nothing -- the three arrays then come back filled with the byte 0xA5 the entry put into the device
 * buffers before the launch.  1: more distinct symbols than the kernel's heap holds (1024); 2: a code word beyond 32 bits; 3: an empty histogram;
 * 4: out_tree_cap too small.  The return value is SZHIP_OK whenever the kernel ran.
 */
typedef struct szhip_book_record {
    uint32_t n_nodes;       /* nodes of the tree: 2 * distinct symbols - 1 */
    uint32_t tree_bytes;    /* serialised size */
    uint32_t max_len;       /* longest code word, bits */
    uint32_t status;
    uint64_t total_bits;    /* sum of count x code length */
    uint64_t total_unpred;  /* hist[0] */
} szhip_book_record;
int szhip_huff_book(szhip_ctx *ctx, const void *hist, unsigned intervals, unsigned char *out_tree, size_t out_tree_cap,
                    uint64_t *out_code64, uint8_t *out_len8, szhip_book_record *record);

/*
 * The copy-shaped passes of the drop-in calls for device-resident arrays (include/sz.h: SZ_hip_compress_device, SZ_hip_decompress_device; kernels in
 * sz_amd/csrc/szh_store.h).  What SZ_compress_args / SZ_decompress do with host loops over the whole array:
 *   szhip_store_be  the raw store (SZ_compress_args_float_StoreOriData, sz_float.c:526-552): the n values of the device array d_src as big-endian bytes at `dst`
 *                   -- a device BYTE address of any alignment (dst_on_device = 1), or host memory (0: through the context's stream buffer).  zero_replacement:
 *                   NULL, or a HOST pointer to one value of the type that is stored in place of every value equal to zero (the MSST19 raw copy, sz_float_pwr.c:2053-2058).
 *   szhip_load_be   the inverse (szd_float.c:106-118): n big-endian values at the byte address `src` (device, any alignment; or host) into the device array d_out.
 *   szhip_fill      n copies of *value (a HOST pointer to one value) into d_out: the decode of a constant stream (szd_float.c:96-104).
 *   szhip_clamp     protectValueRange (szd_float.c:161-176) on the device array d_data, in place: v < vmin -> vmin, v > vmax -> vmax with the reference's
 *                   comparisons, so a NaN stays; vmin / vmax are narrowed to the data's type.
 * Alignment as above: d_src, d_out, d_data are pointers to VALUES (aligned to their element, else SZHIP_ERR_ARG before anything is launched), `dst` / `src` are BYTE
 * pointers.  The n values are cut at the 16-byte boundaries of the output: whole 16-byte pieces move 16 bytes per lane (the input is read 16 bytes at a time where it is
 * aligned alike, else value by value), the head and tail value by value; a byte address that is not aligned to the element is written / read byte by byte.  Nothing
 * in front of or behind the n values is written and the input is never written.  The calls return when their result is complete.
 * szhip_copy: `bytes` bytes between host and device memory on the context's stream (to_device = 1: dst is device memory), complete on return -- the few header bytes
 * and scalars the drop-in calls move.
 */
int szhip_store_be(szhip_ctx *ctx, int dtype, const void *d_src, size_t n, const void *zero_replacement, unsigned char *dst, int dst_on_device);
int szhip_load_be(szhip_ctx *ctx, int dtype, const unsigned char *src, int src_on_device, size_t n, void *d_out);
int szhip_fill(szhip_ctx *ctx, int dtype, const void *value, size_t n, void *d_out);
int szhip_clamp(szhip_ctx *ctx, int dtype, void *d_data, size_t n, double vmin, double vmax);
int szhip_copy(szhip_ctx *ctx, void *dst, const void *src, size_t bytes, int to_device);

/*
 * AN ARRAY AGAINST ITS DECODED COPY, where both lie: the reference's `sz -a` report (example/sz.c:549-620 float, :735-805 double) and the bound checks a caller of an
 * error-bounded compressor makes next, as ONE read of the two arrays (kernels in sz_amd/csrc/szh_quality.h).  `ori` and `dec` are device or host
 * pointers, each on its own (a host array is staged into a buffer of the context, a host view row by row), aligned to their element and to nothing more; neither is
 * written.  szhip_compare takes two contiguous arrays of n values; szhip_compare_view two boxes of r0 x r1 x r2 values (r0 >= 1), each with its own element pitches in
 * the meaning of the VIEWS above.  Points are numbered row-major within the box, 0 .. n - 1.
 * Per point e = |dec - ori| is formed in the data's type (`float err = fabs(data[i] - ori_data[i])`); everything after that runs in double on exactly converted values.
 * A point whose ori, dec or e is a NaN is EXCLUDED (+inf against +inf too: the difference is a NaN): it is counted in n_excluded, in n_excluded_diff as well when the
 * two bit patterns differ, and takes part in nothing else.  Over the points that take part:
 *   vmin, vmax           of ori;  range = vmax - vmin, for SZHIP_F32 the float difference
 *   max_abs_err          and max_abs_idx, the SMALLEST number of a point that attains it
 *   max_pw_rel_err       max e / |ori| over ori != 0 (a double division; inf / inf is a NaN and counts for nothing, as `if (maxpw_relerr < relerr)` has it)
 *   n_zero_changed       points with ori == 0 and dec != 0 (a point-wise relative bound leaves zeros alone)
 *   n_over_abs           points with e > abs_bound;  n_over_pwr: points with ori != 0 and e / |ori| > pw_rel_bound;  n_over_both: points in both sets;
 *                        first_over_idx: the smallest number of a point in either.  A negative bound is "not asked": its counts are 0.  ABS_OR_PW_REL is violated at
 *                        n_over_both points, ABS_AND_PW_REL at n_over_abs + n_over_pwr - n_over_both.
 *   sum_ori, sum_dec, sum_dec_sq, sum_err_sq   double sums of ori, dec, dec * dec, e * e
 *   cov, var_ori, var_dec   only with SZHIP_Q_CORR (else 0): the centred SUMS sum (ori - m1)(dec - m2), sum (ori - m1)^2, sum (dec - m2)^2 of sz.c:595-597 around
 *                        m1 = sum_ori / N, m2 = sum_dec / N -- a SECOND read of both arrays (the one-pass form cancels on a field whose mean dwarfs its spread)
 *   mse = sum_err_sq / N, psnr = 20 log10(range) - 10 log10(mse), nrmse = sqrt(mse) / range, norm_err = sqrt(sum_err_sq),
 *   ac_eff = (cov / N) / sqrt(var_ori / N) / sqrt(var_dec / N), a NaN without SZHIP_Q_CORR          N = n - n_excluded, the points that take part
 * max_abs_idx / first_over_idx are UINT64_MAX when there is no such point; when every point is excluded vmin and vmax are NaNs and max_abs_err is 0.
 * DETERMINISTIC: which values are added in which order depends on the point count alone -- not on addresses, pitches or timing (no floating-point atomics): two calls
 * on the same input return the same bytes, and a view returns what the call returns on contiguous copies of the two boxes, sums included.
 * SZHIP_ERR_ARG before anything is launched, *q untouched: a null pointer, n == 0 or an empty box, n >= 2^40, pitch1 < r2, pitch0 < r1 * pitch1, a misaligned pointer.
 */
typedef struct szhip_quality {
    uint64_t n, n_excluded, n_excluded_diff, n_zero_changed;
    uint64_t n_over_abs, n_over_pwr, n_over_both;
    uint64_t max_abs_idx, first_over_idx;   /* UINT64_MAX when there is none */
    double   vmin, vmax, max_abs_err, max_pw_rel_err;
    double   sum_ori, sum_dec, sum_dec_sq, sum_err_sq;
    double   cov, var_ori, var_dec;         /* centred SUMS; 0 without SZHIP_Q_CORR */
    double   range, mse, psnr, nrmse, norm_err, ac_eff;
} szhip_quality;
#define SZHIP_Q_CORR 1u
int szhip_compare(szhip_ctx *ctx, int dtype, const void *ori, int ori_on_device, const void *dec, int dec_on_device, size_t n,
                  double abs_bound, double pw_rel_bound, unsigned flags, szhip_quality *q);
int szhip_compare_view(szhip_ctx *ctx, int dtype, const void *ori, int ori_on_device, size_t o_pitch0, size_t o_pitch1,
                       const void *dec, int dec_on_device, size_t d_pitch0, size_t d_pitch1, size_t r0, size_t r1, size_t r2,
                       double abs_bound, double pw_rel_bound, unsigned flags, szhip_quality *q);
/*
 * ... for `count` PAIRS of contiguous arrays of n values each (views: szhip_compare_batch_view, below), each pair against its own bounds (abs_bound[i]; pw_rel_bound[i], or pw_rel_bound == NULL:
 * not asked), in a number of launches, copies and synchronisations that does not grow with `count`: one pass-1 launch with the pair as the grid's second dimension,
 * one final launch with one workgroup per pair, one read-back of `count` records -- and the same again around the per-pair means with SZHIP_Q_CORR.
 * out[i] is BYTE FOR BYTE (memcmp of the struct) what szhip_compare returns for pair i alone, sums included: a pair's workgroups, slots and merge tree are those of the
 * single call (the grid's first dimension is a function of n alone).  The 16-byte-or-value-by-value decision stays per array and per piece, so the two arrays of a
 * pair, and the pairs of a batch, may be aligned differently.  on_device: all 2 x count pointers are device (1) or host (0) pointers; host arrays are staged one behind
 * the other.  Arguments and limits as szhip_minmax_batch (SZHIP_ERR_ARG / SZHIP_ERR_UNSUP, nothing launched, `out` untouched).  stats (may be NULL):
 * quant_kernel_launches counts the pass-1 launches: 1.
 */
int szhip_compare_batch(szhip_ctx *ctx, int dtype, const void *const *ori, const void *const *dec, int count, int on_device, size_t n,
                        const double *abs_bound, const double *pw_rel_bound, unsigned flags, szhip_quality *out, szhip_stats *stats);
/*
 * ... for `count` pairs of BOXES of r0 x r1 x r2 values: every ori[i] lies in an array with the element pitches o_pitch0 / o_pitch1, every dec[i] in one with
 * d_pitch0 / d_pitch1 (common to the batch; the pointers are the boxes' first values).  out[i] is byte for byte szhip_compare_view's record for pair i alone -- which
 * is that of the contiguous copies --, in the launches, copies and synchronisations of the call above.  Contiguous pitches on both sides: the call above, exactly.
 * Boxes on the host are staged packed.  Nothing outside the boxes is read, nothing is written.  Arguments and limits as above plus those of szhip_compare_view.
 */
int szhip_compare_batch_view(szhip_ctx *ctx, int dtype, const void *const *ori, size_t o_pitch0, size_t o_pitch1, const void *const *dec, size_t d_pitch0,
                             size_t d_pitch1, int count, int on_device, size_t r0, size_t r1, size_t r2, const double *abs_bound, const double *pw_rel_bound,
                             unsigned flags, szhip_quality *out, szhip_stats *stats);

/* test/diagnostic hook: copy the first `bytes` bytes of an internal device workspace of the LAST call to host.
 * which: 0 coef (T SoA[4][nblocks]) 1 blk_lor (u8) 2 codes in natural order (u16) 3 codes in block order (u16)
 *        4 code histogram (u32) 5 per-column zero counts (u32) 6 per-column unpredictable offsets (u64)
 *        7 unpredictable values (T) 8 stream buffer 12 the input buffer (szhip_stage_input, szhip_pack_view) 13 the blob of szhip_compress_omp_batch */
int szhip_debug_fetch(szhip_ctx *ctx, int which, void *dst, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
