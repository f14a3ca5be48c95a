/*
 * sz.h -- public C API of the MI355X-native SZ 2.1 build.
 *
 * This header declares, with the same names, argument order and struct layouts, the part of the
 * reference's libSZ interface that fronts the GPU hot path, so that existing callers compile
 * against it unchanged (reference: sz/include/sz.h and sz/include/defines.h; each item cites the
 * line it mirrors).  The implementation behind it (sz_amd/csrc/sz_api.c, C) derives the absolute
 * bound, frames the stream and calls the HIP layer declared in szhip.h.
 *
 * Covered: SZ_FLOAT / SZ_DOUBLE; 1-D, 2-D, 3-D arrays and 4-D arrays on the SZ 2.1 path (folded to 3-D as
 * the reference does); withRegression = YES (SZ 2.1 stream) and NO (SZ 1.4 TightDataPointStorage
 * container, 1-D .. 3-D); error-bound modes ABS, REL/VR_REL, ABS_AND_REL, ABS_OR_REL, PSNR, NORM and
 * the point-wise relative family PW_REL, ABS_AND/OR_PW_REL, REL_AND/OR_PW_REL in both of the
 * reference's forms; the zstd / gzip lossless stage of szMode; protectValueRange.
 * Not covered (an explicit error, never a silent CPU fallback): integer types, the time-step and
 * random-access modes, withRegression = NO for 4-D arrays.
 */
#ifndef _SZ_H
#define _SZ_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* sz/include/defines.h:13-17 */
#define SZ_VERNUM 0x0200
#define SZ_VER_MAJOR 2
#define SZ_VER_MINOR 1
#define SZ_VER_BUILD 12
#define SZ_VER_REVISION 4

/* sz/include/defines.h:19-22 */
#define PASTRI 103
#define HZ 102
#define SZ 101
#define SZ_Transpose 104

#define MIN_NUM_OF_ELEMENTS 20 /* defines.h:27 */

/* error-bound modes, defines.h:29-41 */
#define ABS 0
#define REL 1
#define VR_REL 1
#define ABS_AND_REL 2
#define ABS_OR_REL 3
#define PSNR 4
#define NORM 5
#define PW_REL 10
#define ABS_AND_PW_REL 11
#define ABS_OR_PW_REL 12
#define REL_AND_PW_REL 13
#define REL_OR_PW_REL 14

/* data types, defines.h:43-52 */
#define SZ_FLOAT 0
#define SZ_DOUBLE 1
#define SZ_UINT8 2
#define SZ_INT8 3
#define SZ_UINT16 4
#define SZ_INT16 5
#define SZ_UINT32 6
#define SZ_INT32 7
#define SZ_UINT64 8
#define SZ_INT64 9

#define LITTLE_ENDIAN_DATA 0
#define BIG_ENDIAN_DATA 1
#define LITTLE_ENDIAN_SYSTEM 0
#define BIG_ENDIAN_SYSTEM 1

/* defines.h:67-73 */
#define SZ_BEST_SPEED 0
#define SZ_BEST_COMPRESSION 1
#define SZ_DEFAULT_COMPRESSION 2
#define SZ_TEMPORAL_COMPRESSION 3
#define SZ_NO_REGRESSION 0
#define SZ_WITH_LINEAR_REGRESSION 1

#define SZ_PWR_MIN_TYPE 0
#define SZ_PWR_AVG_TYPE 1
#define SZ_PWR_MAX_TYPE 2

/* status codes, defines.h:84-90 */
#define SZ_SCES 0
#define SZ_NSCS -1
#define SZ_FERR -2
#define SZ_TERR -3
#define SZ_DERR -4
#define SZ_MERR -5
#define SZ_BERR -6

#define MetaDataByteLength 28        /* defines.h:97 */
#define MetaDataByteLength_double 36 /* defines.h:98 */

#define GZIP_COMPRESSOR 0 /* defines.h:103 */
#define ZSTD_COMPRESSOR 1

/* sz/include/sz.h:164-198 -- field order and types are ABI */
typedef struct sz_params
{
	int dataType;
	unsigned int max_quant_intervals;
	unsigned int quantization_intervals;
	unsigned int maxRangeRadius;
	int sol_ID;
	int losslessCompressor;
	int sampleDistance;
	float predThreshold;
	int szMode;
	int gzipMode;
	int errorBoundMode;
	double absErrBound;
	double relBoundRatio;
	double psnr;
	double normErr;
	double pw_relBoundRatio;
	int segment_size;
	int pwr_type;

	int protectValueRange;
	float fmin, fmax;
	double dmin, dmax;

	int snapshotCmprStep;
	int predictionMode;

	int accelerate_pw_rel_compression;
	int plus_bits;

	int randomAccess;
	int withRegression;
} sz_params;

/* sz/include/sz.h:200-209 */
typedef struct sz_metadata
{
	int versionNumber[3];
	int isConstant;
	int isLossless;
	int sizeType;
	size_t dataSeriesLength;
	int defactoNBBins;
	struct sz_params* conf_params;
} sz_metadata;

/* sz/include/sz.h:211-217 */
typedef struct sz_exedata
{
	char optQuantMode;
	int intvCapacity;
	int intvRadius;
	unsigned int SZ_SIZE_TYPE;
} sz_exedata;

/* globals that callers poke directly (example/sz.c:317-338), sz/include/sz.h:232-240 */
extern int versionNumber[4];
extern int dataEndianType;
extern int sysEndianType;
extern sz_params *confparams_cpr;
extern sz_params *confparams_dec;
extern sz_exedata *exe_params;

/* sz/include/sz.h:255-334 */
int SZ_Init(const char *configFilePath);
int SZ_Init_Params(sz_params *params);
size_t computeDataLength(size_t r5, size_t r4, size_t r3, size_t r2, size_t r1);
int computeDimension(size_t r5, size_t r4, size_t r3, size_t r2, size_t r1);
int filterDimension(size_t r5, size_t r4, size_t r3, size_t r2, size_t r1, size_t* correctedDimension);

unsigned char *SZ_compress(int dataType, void *data, size_t *outSize, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1);
unsigned char* SZ_compress_args(int dataType, void *data, size_t *outSize, int errBoundMode, double absErrBound,
double relBoundRatio, double pwrBoundRatio, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1);
int SZ_compress_args2(int dataType, void *data, unsigned char* compressed_bytes, size_t *outSize,
int errBoundMode, double absErrBound, double relBoundRatio, double pwrBoundRatio,
size_t r5, size_t r4, size_t r3, size_t r2, size_t r1);

void *SZ_decompress(int dataType, unsigned char *bytes, size_t byteLength, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1);
size_t SZ_decompress_args(int dataType, unsigned char *bytes, size_t byteLength, void* decompressed_array, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1);

sz_metadata* SZ_getMetadata(unsigned char* bytes);
/* what the reference's command-line tool (example/sz.c:498-845) calls next to the API: sz.c:768, utility.c:156, :216, :236 */
void SZ_printMetadata(sz_metadata* metadata);
int is_lossless_compressed_data(unsigned char* compressedBytes, size_t cmpSize);
uint64_t sz_lossless_decompress65536bytes(int losslessCompressor, unsigned char* compressBytes, uint64_t cmpSize, unsigned char** oriData);
void* detransposeData(void* data, int dataType, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1);
void SZ_Finalize(void);

void convertSZParamsToBytes(sz_params* params, unsigned char* result);
void convertBytesToSZParams(unsigned char* bytes, sz_params* params);

unsigned char* SZ_compress_customize(const char* appName, void* userPara, int dataType, void* data, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1, size_t *outSize, int *status);
unsigned char* SZ_compress_customize_threadsafe(const char* cmprName, void* userPara, int dataType, void* data, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1, size_t *outSize, int *status);
void* SZ_decompress_customize(const char* appName, void* userPara, int dataType, unsigned char* bytes, size_t byteLength, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1, int* status);
void* SZ_decompress_customize_threadsafe(const char* cmprName, void* userPara, int dataType, unsigned char* bytes, size_t byteLength, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1, int *status);

/* ---- additive entry points of this build (not in the reference) ---- */
/* device that SZ_* calls run on (default: env SZ_HIP_DEVICE or 0); call before the first compress */
int SZ_hip_set_device(int device);

/* The reference's OpenMP container for 3-D arrays (sz/include/sz_omp.h:26, :29, :36, :40): same names, arguments and stream as an OpenMP
 * build of libSZ.  r1 is the slowest dimension here, as in sz_omp.c.  `comp_data` of the inverse: the stream behind its first
 * 4 + MetaDataByteLength bytes (example/sz_openmp.c:580).  SZ_hip_set_omp_threads: the box count (omp_get_max_threads() of an OpenMP
 * build; 0 = pick one: boxes of at most 32768 points); the HIP layer's restrictions are in include/szhip.h (szhip_compress_omp). */
void SZ_hip_set_omp_threads(int thread_num);
/* sz_omp.h:44-47 of an OpenMP build (sz_omp.c:14-53): sz_set_num_threads sets the box count like SZ_hip_set_omp_threads; the 1-D / 2-D entry
 * points below are stubs in the reference itself (they return NULL / do nothing, sz_omp.c:56-61, :360-364, :570-576, :866-870) */
void sz_set_num_threads(int nthreads);
int sz_get_max_threads(void);
int sz_get_thread_num(void);
double sz_wtime(void);
unsigned char *SZ_compress_float_1D_MDQ_openmp(float *oriData, size_t r1, double realPrecision, size_t *comp_size);
unsigned char *SZ_compress_float_2D_MDQ_openmp(float *oriData, size_t r1, size_t r2, double realPrecision, size_t *comp_size);
unsigned char *SZ_compress_double_1D_MDQ_openmp(double *oriData, size_t r1, double realPrecision, size_t *comp_size);
unsigned char *SZ_compress_double_2D_MDQ_openmp(double *oriData, size_t r1, size_t r2, double realPrecision, size_t *comp_size);
void decompressDataSeries_float_1D_openmp(float **data, size_t r1, unsigned char *comp_data);
void decompressDataSeries_float_2D_openmp(float **data, size_t r1, size_t r2, unsigned char *comp_data);
void decompressDataSeries_double_1D_openmp(double **data, size_t r1, unsigned char *comp_data);
void decompressDataSeries_double_2D_openmp(double **data, size_t r1, size_t r2, unsigned char *comp_data);
unsigned char *SZ_compress_float_3D_MDQ_openmp(float *oriData, size_t r1, size_t r2, size_t r3, float realPrecision, size_t *comp_size);
unsigned char *SZ_compress_double_3D_MDQ_openmp(double *oriData, size_t r1, size_t r2, size_t r3, double realPrecision, size_t *comp_size);
void decompressDataSeries_float_3D_openmp(float **data, size_t r1, size_t r2, size_t r3, unsigned char *comp_data);
void decompressDataSeries_double_3D_openmp(double **data, size_t r1, size_t r2, size_t r3, unsigned char *comp_data);
/* Many small arrays of ONE shape r1 x r2 x r3 and type in one call (szhip_compress_omp_batch / szhip_decompress_omp_batch of szhip.h: one set of kernel launches over
 * the boxes of all arrays instead of one blocking call per array).  data[i]: the arrays, on the host or -- data_on_device -- on the device; realPrecision[i]: the
 * absolute bound of array i.  streams[i] comes back as a malloc'd stream (caller frees) of comp_sizes[i] bytes, byte for byte what
 * SZ_compress_{float,double}_3D_MDQ_openmp returns for array i under the same configuration: the same parameter bytes of confparams_cpr, the same box count
 * (sz_set_num_threads / SZ_HIP_OMP_THREADS, else picked from the shape), the body behind 4 + MetaDataByteLength bytes.  The inverse takes comp_data[i] at the stream's
 * FIRST byte, as returned (it skips the parameter bytes itself), comp_sizes[i] bytes long, and writes array i to out[i] (host, or device with out_on_device).
 * Both return SZ_SCES, or SZ_NSCS with a printed reason; when any array fails every returned stream is freed and its pointer nulled.
 * These two take an absolute bound per array and write unmarked streams, as the `*_openmp` entry points do (never wrapped by the lossless stage); the range-based
 * modes and the streams of SZ_compress_args under SZ_HIP_MODE=omp are SZ_hip_compress_args_batch's, below. */
int SZ_hip_compress_openmp_batch(int dataType, int count, const void *const *data, int data_on_device, const double *realPrecision,
                                 size_t r1, size_t r2, size_t r3, unsigned char **streams, size_t *comp_sizes);
int SZ_hip_decompress_openmp_batch(int dataType, int count, unsigned char *const *comp_data, const size_t *comp_sizes, void *const *out, int out_on_device,
                                   size_t r1, size_t r2, size_t r3);
/* A sub-box of a 3-D array out of its stream: start / end per dimension in the order r3, r2, r1 (slowest first), end exclusive.  Returns a malloc'd array of
 * (end[0]-start[0]) x (end[1]-start[1]) x (end[2]-start[2]) values (caller frees), bit for bit that part of what SZ_decompress returns; NULL with a printed
 * reason otherwise.  Reads what this library's SZ_decompress recognises as an OpenMP container: the streams SZ_compress_args writes for 3-D arrays under
 * SZ_HIP_MODE=omp, where every box decodes on its own -- only the boxes that meet the region are decoded (szhip_decompress_omp_region; boxes outside it are
 * not validated).  A stream wrapped by the zstd or gzip stage (szMode other than SZ_BEST_SPEED) has to be unwrapped WHOLE first: only the decode is partial
 * then.  Every other stream (SZ 2.1, SZ 1.4, constant, raw, not 3-D) is refused with a message that names SZ_HIP_MODE=omp.  An unmarked stream of the
 * `*_openmp` entry points goes to szhip_decompress_omp_region (szhip.h) with its body offset. */
void *SZ_hip_decompress_region(int dataType, unsigned char *bytes, size_t byteLength, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1,
                               const size_t start[3], const size_t end[3]);
/* The opposite direction: a sub-box of a larger 3-D HOST array compressed from, and decoded into, where it lies.  r5 .. r1 are the extents of the PARENT
 * (r5 = r4 = 0); start / end as above.  SZ_hip_compress_region returns exactly what SZ_compress_args returns for a contiguous copy of the sub-box under the same
 * configuration -- every error-bound mode (the range is the sub-box's), SZ 2.1, SZ 1.4 and SZ_HIP_MODE=omp, the lossless stage, the constant and raw-store rules --
 * without the caller making that copy: only the sub-box's rows go to the device (szhip_pack_view, szhip.h).  SZ_hip_decompress_into_region decodes a stream of the
 * sub-box's extents (anything SZ_decompress reads) into the parent and writes nothing outside the sub-box; SZ_SCES, or SZ_NSCS with nothing written.  Anything but a
 * 3-D parent, or an empty or out-of-range box, gives NULL / SZ_NSCS with a printed reason.  (The reference's SZ_compress_args3 is not provided: INTEGRATION.md.) */
unsigned char *SZ_hip_compress_region(int dataType, void *data, size_t *outSize, int errBoundMode, double absErrBound, double relBoundRatio, double pwrBoundRatio,
                                      size_t r5, size_t r4, size_t r3, size_t r2, size_t r1, const size_t start[3], const size_t end[3]);
int SZ_hip_decompress_into_region(int dataType, unsigned char *bytes, size_t byteLength, void *parent, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1,
                                  const size_t start[3], const size_t end[3]);
/* An array that is already on the GPU, and a stream that may stay there.  Pointer kinds are taken on trust from the arguments, and the ordering contract is szhip.h's:
 * whatever produced the array or the stream is synchronised by the caller first; the calls return when their results are complete.  Configuration (SZ_Init, confparams_cpr)
 * and SZ_hip_last_stats behave as for SZ_compress_args / SZ_decompress on the calling thread.
 * SZ_hip_compress_device: everything SZ_compress_args does, for an array in DEVICE memory (aligned to its element); the stream comes back as malloc'd host memory, byte for
 * byte what SZ_compress_args returns for a host copy of the array under the same configuration -- every error-bound mode, SZ 2.1 and withLinearRegression = NO, 1-D to 4-D,
 * SZ_HIP_MODE=omp, protectValueRange, the constant, <= 20-value and raw-store rules, the lossless stage (on the host, on the finished stream) -- and NULL with the same
 * message for whatever SZ_compress_args refuses.  The array is never written and never copied to the host: on the input side only scalars cross the bus (the range, the first
 * value of a constant array, the <= 20 values, the sign bytes of the PW_REL forms); the raw store is a kernel (szhip_store_be).
 * SZ_hip_compress_device_into: the same stream into the caller's DEVICE buffer d_stream of `capacity` bytes (any alignment), *outSize = its length; nothing outside
 * [d_stream, d_stream + capacity) is written; bytes of the buffer behind the stream are undefined.  SZ_SCES, or SZ_NSCS with a printed reason: a capacity below the stream's
 * length (the context stays usable), and any configuration whose szMode is not SZ_BEST_SPEED -- the lossless stage is host code, so a stream that has to pass it is
 * returned by SZ_hip_compress_device instead.
 * SZ_hip_decompress_device: everything SZ_decompress reads (SZ 2.1, SZ 1.4, both PW_REL forms, the marked OpenMP container, constant, raw and <= 20-value streams, the
 * protectValueRange clamp), decoded bit for bit into the caller's DEVICE array d_out (aligned to its element): exactly the array's values are written and nothing else.  The
 * stream lies on the host (bytes_on_device = 0) or on the device (1, any alignment): of a device stream only its first 256 bytes (the header fields) and the sign bytes of
 * a PW_REL container come to the host, the payload is read where it lies.  A zstd / gzip-wrapped stream that lies on the device is brought down WHOLE, unwrapped on the host
 * and decoded from there: that stage is host code.  SZ_SCES, or SZ_NSCS with the reason SZ_decompress prints; on failure the contents of d_out are undefined. */
unsigned char *SZ_hip_compress_device(int dataType, const void *d_data, size_t *outSize, int errBoundMode, double absErrBound,
                                      double relBoundRatio, double pwrBoundRatio, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1);
int SZ_hip_compress_device_into(int dataType, const void *d_data, unsigned char *d_stream, size_t capacity, size_t *outSize, int errBoundMode,
                                double absErrBound, double relBoundRatio, double pwrBoundRatio, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1);
int SZ_hip_decompress_device(int dataType, const unsigned char *bytes, int bytes_on_device, size_t byteLength, void *d_out,
                             size_t r5, size_t r4, size_t r3, size_t r2, size_t r1);
/* An array against its decoded copy: the reference's `-a` report (example/sz.c:549-620) and the bound checks, computed on the device in one read of the two arrays
 * (szhip_compare of szhip.h, which describes every field of struct szhip_quality; NaN points are excluded and counted).  SZ_hip_compare: two HOST arrays of
 * r5 x ... x r1 values (unused dimensions 0); SZ_hip_compare_device: two DEVICE arrays, aligned to their element, complete when the call is made; neither is written.
 * absBound / pwRelBound: the bounds the n_over_* counts are taken against, negative for "not asked"; flags: SZHIP_Q_CORR for the correlation (acEff), which costs a
 * second read.  SZ_SCES, or SZ_NSCS with a printed reason (a null pointer, no points, a misaligned pointer), *out untouched.
 * SZ_hip_print_quality prints the lines of that report in the reference's formats; cmp_bytes: the stream's length for the compressionRatio line (0: no such line);
 * the acEff line appears when the correlation was asked for. */
struct szhip_quality;
int SZ_hip_compare(int dataType, const void *ori, const void *dec, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1, double absBound, double pwRelBound,
                   int flags, struct szhip_quality *out);
int SZ_hip_compare_device(int dataType, const void *d_ori, const void *d_dec, size_t r5, size_t r4, size_t r3, size_t r2, size_t r1, double absBound,
                          double pwRelBound, int flags, struct szhip_quality *out);
void SZ_hip_print_quality(const struct szhip_quality *q, size_t cmp_bytes, int is_double);
/* SZ_compress_args over MANY 3-D arrays of one shape r1 x r2 x r3 (r1 slowest, as SZ_hip_compress_openmp_batch) and type in one call, with its inverse and the error
 * report over the round trip.
 * SZ_hip_compress_args_batch: errBoundMode is ABS, REL, ABS_AND_REL, ABS_OR_REL, PSNR or NORM (psnr and normErr from the configuration); every array's value range
 * comes from ONE launch (szhip_minmax_batch), its bound from the rule SZ_compress_args applies, its own range and the call's absErrBound / relBoundRatio.  streams[i]
 * (malloc'd, caller frees; comp_sizes[i] bytes) is byte for byte what SZ_compress_args of this library returns under SZ_HIP_MODE=omp for array i ALONE -- the same
 * configuration and arguments, as the first call after the same SZ_Init (a PSNR call rewrites confparams_cpr->errorBoundMode, as the reference does) -- including the
 * parameter bytes, which carry the item's own bound and range, and the mark in byte 19.  The call does not read SZ_HIP_MODE: it always writes this form.
 * Arrays with range > bound > 0 go through one szhip_compress_omp_batch with per-item bounds and parameter bytes (batched[i] = 1; batched may be NULL); an array
 * with range <= bound (a constant array, or two values closer than an ABS bound) gets the reference's constant stream -- of a device array only its first value
 * crosses the bus; a bound that is not positive takes SZ_compress_args' ordinary path from inside the call (both batched[i] = 0).  A host array crosses the bus once.
 * SZ_NSCS with a printed reason and nothing launched: a mode >= PW_REL, a configuration whose szMode is not SZ_BEST_SPEED (the lossless stage is host code) or that
 * asks for random access, a shape with an extent below 2, of at most 20 values or for which no box grid is found (SZ_HIP_OMP_THREADS / sz_set_num_threads as for
 * SZ_HIP_MODE=omp).  When an item fails its stream is NULL, the others are delivered, and the call returns SZ_NSCS.
 * SZ_hip_decompress_batch takes what that call returns (host streams): the streams SZ_decompress recognises as marked containers, with the box count of the first of
 * them, go through one szhip_decompress_omp_batch; everything else -- constant streams, a container of another box count, an SZ 2.1 stream -- through SZ_decompress'
 * own path, stream by stream.  out[i] (host, or device with out_on_device; aligned to its element) receives bit for bit what SZ_decompress returns for stream i.  A
 * failing item does not disturb the others; the call returns SZ_NSCS if any item failed.
 * SZ_hip_compare_batch: szhip_compare_batch (szhip.h) on `count` pairs of r1 x r2 x r3 values, pair i against absBound[i] and pwRelBound[i] (pwRelBound NULL: not
 * asked): out[i] is byte for byte SZ_hip_compare's record for pair i.
 * SZ_hip_last_stats after each call: the stats of its shared launches (quant_kernel_launches: the sweep launches, one per form; the pass-1 launches of the report).
 * ARRAYS OF DIFFERENT SHAPES: SZ_hip_compress_args_batch_shapes / SZ_hip_decompress_batch_shapes are the two calls above with the extents per
 * item, dims[3 i], dims[3 i + 1], dims[3 i + 2] = r1, r2, r3 of array i (r1 slowest).  The contracts hold item by item: streams[i] is byte for byte what
 * SZ_compress_args returns under SZ_HIP_MODE=omp for array i alone -- its box count from the rule that mode applies to ITS shape (sz_set_num_threads /
 * SZ_HIP_OMP_THREADS, else picked from the shape), its range from ONE szhip_minmax_batch_lens, its bound from SZ_compress_args' rule --, through one
 * szhip_compress_omp_batch_shapes; the decode puts every marked container, whatever its box count, through one szhip_decompress_omp_batch_shapes.  An item of at most
 * 20 values, with an extent below 2 or without a box grid takes SZ_compress_args' ordinary path from inside the call (batched[i] = 0) instead of refusing it; the
 * refusals of the whole call are otherwise those above, and an extent of 0 or an array of 2^32 values or more.
 * Not covered: the lossless stage, point-wise relative modes, the slab container, compressing arrays of different shapes that are sub-boxes (decoding sub-boxes of streams of any shapes: SZ_hip_decompress_batch_regions below), arrays of different types or not 3-D, the
 * error report over pairs of different lengths (SZ_hip_compare_batch is element-wise: group the pairs by shape); sub-boxes of one shape: the three *_region calls below. */
int SZ_hip_compress_args_batch(int dataType, int count, const void *const *data, int data_on_device, int errBoundMode, double absErrBound, double relBoundRatio,
                               size_t r1, size_t r2, size_t r3, unsigned char **streams, size_t *comp_sizes, int *batched);
int SZ_hip_decompress_batch(int dataType, int count, unsigned char *const *bytes, const size_t *byteLengths, void *const *out, int out_on_device,
                            size_t r1, size_t r2, size_t r3);
int SZ_hip_compress_args_batch_shapes(int dataType, int count, const void *const *data, int data_on_device, int errBoundMode, double absErrBound, double relBoundRatio,
                                      const size_t *dims, unsigned char **streams, size_t *comp_sizes, int *batched);
int SZ_hip_decompress_batch_shapes(int dataType, int count, unsigned char *const *bytes, const size_t *byteLengths, void *const *out, int out_on_device,
                                   const size_t *dims);
int SZ_hip_compare_batch(int dataType, int count, const void *const *ori, const void *const *dec, int on_device, size_t r1, size_t r2, size_t r3,
                         const double *absBound, const double *pwRelBound, int flags, struct szhip_quality *out);
/* SUB-BOXES OF MANY STREAMS in one call: SZ_hip_decompress_region per item, into destinations that may be views -- the faces of neighbouring
 * patches into ghost layers, slices through a level.  Item i: the host stream bytes[i] of byteLengths[i] bytes of an array of dims[3 i .. 3 i + 2] = r1, r2, r3 values
 * (laid out as in SZ_hip_decompress_batch_shapes), its sub-box start[3 i ..] / end[3 i ..] (the dimension order of SZ_hip_decompress_region: slowest first, end
 * exclusive), and the destination out[i] (host, or device with out_on_device; aligned to its element): contiguous when out_pitches is NULL, else with the two ELEMENT
 * pitches out_pitches[2 i] (between planes) and out_pitches[2 i + 1] (between rows) of szhip.h's views.  The destination sub-box receives bit for bit that part of what
 * SZ_decompress returns for the stream, and no other byte of the destination's allocation is written.
 * Marked containers -- what SZ_compress_args writes under SZ_HIP_MODE=omp and the SZ_hip_compress_args_batch* calls write -- go through ONE
 * szhip_decompress_omp_batch_region: only the boxes the regions meet are decoded, several regions of one stream (the same bytes[i]) share its header work, and the
 * number of launches and synchronisations does not grow with `count`.  A constant stream (the batch compress calls write them for constant patches) fills its region
 * with the value SZ_decompress gives.  A stream wrapped by the zstd or gzip stage is unwrapped WHOLE first.  Every other stream (SZ 2.1, SZ 1.4, point-wise relative,
 * raw, not 3-D) is refused for that item alone with the printed reason of SZ_hip_decompress_region: the others are delivered and the call returns SZ_NSCS.
 * SZ_NSCS with nothing written: null arguments, a type other than float or double, an empty or out-of-range box, pitches below the region's extents.
 * Not covered: device-resident streams (szhip_decompress_omp_batch_region takes them), a type per item, the slab container. */
int SZ_hip_decompress_batch_regions(int dataType, int count, unsigned char *const *bytes, const size_t *byteLengths, const size_t *dims, const size_t *start,
                                    const size_t *end, void *const *out, int out_on_device, const size_t *out_pitches);
/* ---- the three calls above on ONE BOX [start, end) common to `count` 3-D parents of r1 x r2 x r3 values (r1 slowest; start / end as in SZ_hip_compress_region): the
 * interiors of patches with ghost layers.  parents[i] points at parent i's first value; the ghost cells are neither read into a stream or a
 * range nor written.
 * SZ_hip_compress_args_batch_region: streams[i] is byte for byte what SZ_hip_compress_args_batch returns for contiguous copies of the sub-boxes -- the same modes,
 * refusals (on the sub-box's extents) and per-item failure rule.  The range is the sub-box's own, from ONE szhip_minmax_batch_view launch; the items with
 * range > bound > 0 go through one szhip_compress_omp_batch_view; a constant sub-box gets the reference's constant stream (of a device parent only the sub-box's
 * first value crosses the bus); a bound that is not positive takes SZ_compress_args' ordinary path from a packed copy of that one item (szhip_pack_view).  Of host
 * parents only the sub-boxes' rows cross the bus, once for the ranges and once for the streams.
 * SZ_hip_decompress_batch_into_region accepts what SZ_hip_decompress_batch accepts and writes into sub-box i bit for bit what that call writes into out[i], and no
 * other byte of a parent: containers through one szhip_decompress_omp_batch_view, every other stream (constant streams among them) decoded whole and then placed
 * through the pitches (szhip_scatter_view for a device parent); of a stream that fails nothing reaches its parent.
 * SZ_hip_compare_batch_region: szhip_compare_batch_view on the sub-boxes of ori_parents[i] and dec_parents[i]; out[i] is byte for byte SZ_hip_compare's record of
 * contiguous copies of pair i.
 * SZ_NSCS with a printed reason and nothing launched or written: a null parent, a parent that is not 3-D, start[d] >= end[d] or end[d] beyond the extent. */
int SZ_hip_compress_args_batch_region(int dataType, int count, const void *const *parents, int data_on_device, int errBoundMode, double absErrBound,
                                      double relBoundRatio, size_t r1, size_t r2, size_t r3, const size_t start[3], const size_t end[3],
                                      unsigned char **streams, size_t *comp_sizes, int *batched);
int SZ_hip_decompress_batch_into_region(int dataType, int count, unsigned char *const *bytes, const size_t *byteLengths, void *const *parents, int out_on_device,
                                        size_t r1, size_t r2, size_t r3, const size_t start[3], const size_t end[3]);
int SZ_hip_compare_batch_region(int dataType, int count, const void *const *ori_parents, const void *const *dec_parents, int on_device, size_t r1, size_t r2, size_t r3,
                                const size_t start[3], const size_t end[3], const double *absBound, const double *pwRelBound, int flags, struct szhip_quality *out);
/* per-call measurements of the last SZ_compress_args / SZ_decompress on this thread's context; see szhip.h */
struct szhip_stats;
int SZ_hip_last_stats(struct szhip_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* _SZ_H */
