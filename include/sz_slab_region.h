/*
 * sz_slab_region.h -- a sub-box of the array in a slab container (sz_slab.h), without decoding the slabs and boxes it does not meet.  Included by sz_slab.h:
 * a caller of the container needs no other header.  (A header of its own because sz_slab.h's seven entry points are the container's write / read interface that
 * sz_amd/slab.py mirrors; this one rests on SZ_hip_decompress_region of sz.h, which only this library has.)
 */
#ifndef SZ_SLAB_REGION_H
#define SZ_SLAB_REGION_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the sub-box [start, end) (per dimension, slowest first, end exclusive) of a container's array as one malloc'd array (caller frees); NULL on error.
 * The container is checked as by sz_slab_decompress; only the slabs that meet [start[0], end[0]) are touched.  A slab whose sub-stream is an OpenMP
 * container (SZ_compress_args under SZ_HIP_MODE=omp, where the box grid divides the slab) goes through SZ_hip_decompress_region with dim 0 translated to
 * the slab; a slab with any other sub-stream is decoded whole by SZ_decompress and cropped on the host. */
void *sz_slab_decompress_region(const unsigned char *blob, size_t len, const size_t start[3], const size_t end[3], int *dataType);

#ifdef __cplusplus
}
#endif
#endif
