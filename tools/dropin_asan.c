/* dropin_asan.c -- a stand-alone driver of the drop-in calls for device-resident arrays (include/sz.h) over the HIP-on-CPU shim (tests/sim), for a host
 * sanitizer build: one SZ_hip_compress_device / SZ_hip_compress_device_into / SZ_hip_decompress_device round per stream kind on the shim's "device" memory, which
 * is host memory -- every array, stream and buffer a malloc of exactly its size, so that the sanitizer sees any byte read or written outside it.
 * tools/dropin_asan.sh builds it with -fsanitize=address,undefined and runs it.  Never built for, or run on, a GPU. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sz.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s: ", kind); printf(__VA_ARGS__); printf("\n"); failures++; return; } } while (0)

typedef struct { int withRegression, protect, accelerate, szMode; const char *omp; } conf_t;
static void reinit(const conf_t *c)
{
    SZ_Init(NULL);
    confparams_cpr->szMode = c->szMode; confparams_cpr->withRegression = c->withRegression; confparams_cpr->protectValueRange = c->protect;
    confparams_cpr->accelerate_pw_rel_compression = c->accelerate;
    if (c->omp) setenv("SZ_HIP_MODE", c->omp, 1); else unsetenv("SZ_HIP_MODE");
}

static void round_trip(const char *kind, const conf_t *c, int dataType, const void *x, size_t r3, size_t r2, size_t r1, int mode, double abs_, double pwr)
{
    const size_t esz = dataType == SZ_FLOAT ? 4 : 8, n = (r3 ? r3 : 1) * (r2 ? r2 : 1) * r1;
    size_t len = 0, dlen = 0, ilen = 0;
    reinit(c);
    unsigned char *want = SZ_compress_args(dataType, (void *)x, &len, mode, abs_, 0.0, pwr, 0, 0, r3, r2, r1);
    CHECK(want, "SZ_compress_args returned NULL");
    void *d_x = malloc(n * esz);                                  /* the "device" array */
    memcpy(d_x, x, n * esz);
    reinit(c);
    unsigned char *got = SZ_hip_compress_device(dataType, d_x, &dlen, mode, abs_, 0.0, pwr, 0, 0, r3, r2, r1);
    CHECK(got && dlen == len && memcmp(got, want, len) == 0, "SZ_hip_compress_device: %zu bytes against %zu, or other bytes", dlen, len);
    CHECK(memcmp(d_x, x, n * esz) == 0, "the input was written");
    if (c->szMode == SZ_BEST_SPEED) {
        unsigned char *whole = (unsigned char *)malloc(len + 1);  /* the stream buffer one byte behind an aligned address, exactly the stream's length */
        reinit(c);
        int rc = SZ_hip_compress_device_into(dataType, d_x, whole + 1, len, &ilen, mode, abs_, 0.0, pwr, 0, 0, r3, r2, r1);
        CHECK(rc == SZ_SCES && ilen == len && memcmp(whole + 1, want, len) == 0, "SZ_hip_compress_device_into: rc %d, %zu bytes against %zu, or other bytes", rc, ilen, len);
        if (len > 1) {
            reinit(c);
            rc = SZ_hip_compress_device_into(dataType, d_x, whole + 1, len - 1, &ilen, mode, abs_, 0.0, pwr, 0, 0, r3, r2, r1);
            CHECK(rc == SZ_NSCS, "a capacity of length - 1 was not refused");
        }
        free(whole);
    }
    void *ref = SZ_decompress(dataType, want, len, 0, 0, r3, r2, r1);
    CHECK(ref, "SZ_decompress returned NULL");
    for (int on_device = 0; on_device < 2; on_device++) {
        unsigned char *s = (unsigned char *)malloc(len + 3);      /* the stream at byte 3 of its allocation */
        memcpy(s + 3, want, len);
        void *d_out = malloc(n * esz);
        memset(d_out, 0xA5, n * esz);
        int rc = SZ_hip_decompress_device(dataType, s + 3, on_device, len, d_out, 0, 0, r3, r2, r1);
        CHECK(rc == SZ_SCES && memcmp(d_out, ref, n * esz) == 0, "SZ_hip_decompress_device (stream on the %s): rc %d, or other values", on_device ? "device" : "host", rc);
        free(d_out); free(s);
    }
    const int flag = n > 20 && c->szMode == SZ_BEST_SPEED ? want[3] : 0;
    free(ref); free(got); free(want); free(d_x);
    printf("ok     %s: %zu values, %zu stream bytes, flag byte 0x%02x\n", kind, n, len, flag);
}

int main(void)
{
    enum { A = 12, B = 20, C = 28, N = A * B * C };
    float *s = (float *)malloc(N * sizeof(float)), *noise = (float *)malloc(N * sizeof(float)), *pw = (float *)malloc(N * sizeof(float)), *flat = (float *)malloc(N * sizeof(float));
    double *sd = (double *)malloc(N * sizeof(double));
    unsigned seed = 12345;
    for (int i = 0; i < A; i++) for (int j = 0; j < B; j++) for (int k = 0; k < C; k++) {
        const int at = (i * B + j) * C + k;
        seed = seed * 1664525u + 1013904223u;
        const double u = (seed >> 8) / 16777216.0;
        s[at] = (float)(sin(0.21 * i) * cos(0.17 * j) + 0.5 * sin(0.13 * k + 0.05 * i));
        sd[at] = sin(0.21 * i) * cos(0.17 * j) + 0.5 * sin(0.13 * k + 0.05 * i);
        noise[at] = (float)(u * 2 - 1) * 1000.0f;
        pw[at] = (float)(exp(2.0 * s[at]) * (s[at] + 0.15 < 0 ? -1 : 1));
        if (at % 23 == 5) pw[at] = 0;
        flat[at] = 3.25f;
    }
    const conf_t speed = {1, 0, 1, SZ_BEST_SPEED, NULL}, sz14 = {0, 0, 1, SZ_BEST_SPEED, NULL}, protect = {1, 1, 1, SZ_BEST_SPEED, NULL},
                 logform = {1, 0, 0, SZ_BEST_SPEED, NULL}, omp = {1, 0, 1, SZ_BEST_SPEED, "omp"}, zstd = {1, 0, 1, SZ_BEST_COMPRESSION, NULL};
    round_trip("SZ 2.1, 3-D float32", &speed, SZ_FLOAT, s, A, B, C, ABS, 1e-3, 0);
    round_trip("SZ 2.1, 3-D float64, protectValueRange", &protect, SZ_DOUBLE, sd, A, B, C, ABS, 1e-2, 0);
    round_trip("SZ 2.1, 2-D float32", &speed, SZ_FLOAT, s, 0, A * B, C, ABS, 1e-3, 0);
    round_trip("SZ 1.4, 3-D float32", &sz14, SZ_FLOAT, s, A, B, C, ABS, 1e-3, 0);
    round_trip("1-D float32", &speed, SZ_FLOAT, s, 0, 0, N, ABS, 1e-3, 0);
    round_trip("OpenMP container", &omp, SZ_FLOAT, s, A, B, C, ABS, 1e-3, 0);
    round_trip("PW_REL, MSST19", &speed, SZ_FLOAT, pw, A, B, C, PW_REL, 0, 1e-2);
    round_trip("PW_REL, log domain", &logform, SZ_FLOAT, pw, A, B, C, PW_REL, 0, 1e-2);
    round_trip("raw store", &speed, SZ_FLOAT, noise, A, B, C, ABS, 1e-7, 0);
    round_trip("raw store, MSST19", &speed, SZ_FLOAT, noise, 0, 0, 2000, PW_REL, 0, 1e-5);
    round_trip("constant", &speed, SZ_FLOAT, flat, A, B, C, ABS, 1e-3, 0);
    round_trip("18 values", &speed, SZ_FLOAT, s, 2, 3, 3, ABS, 1e-3, 0);
    round_trip("zstd-wrapped", &zstd, SZ_FLOAT, s, A, B, C, ABS, 1e-3, 0);
    SZ_Finalize();
    free(s); free(noise); free(pw); free(flat); free(sd);
    printf(failures ? "%d kinds FAILED\n" : "all kinds ok\n", failures);
    return failures ? 1 : 0;
}
