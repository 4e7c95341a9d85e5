// Test program (not product code): sf_rootforms.h's forms against the select forms they replace and against the
// correctly rounded sqrtf, over all 2^32 float patterns x. Built and run by tests/test_root_forms_host.py with
// -ffp-contract=off; every fused operation is an explicit fmaf.
//
// The device's v_sqrt_f32 is not available here, so sqrt_fix gets every estimate within 1 ulp of the correctly rounded
// root (the root itself and both neighbours): the hardware's estimate is one of the three.
//
// Prints one line: n_domain bad_fix_vs_select bad_fix_vs_sqrtf n_roots bad_roots n_took_t0
#define SF_ROOTFORMS_HOST
#include "sf_rootforms.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>

// the forms replaced (sf_kernels.hip's near_root_big before, sf_fastmath.h's sqrt_rn_mid)
static inline float sqrt_select(float s0, float x)
{
    const float sdn = sf_rf_float(sf_rf_bits(s0) - 1u);
    const float sup = sf_rf_float(sf_rf_bits(s0) + 1u);
    const float rdn = fmaf(-sdn, s0, x);
    const float rup = fmaf(-sup, s0, x);
    float thc = rdn <= 0.0f ? sdn : s0;
    thc = rup > 0.0f ? sup : thc;
    return thc;
}
static inline float root_select(float tca, float thc)
{
    const float t0 = tca + thc;
    const float t1 = tca - thc;
    return (t0 <= t1) ? t0 : t1;
}

// tca: +-0, the smallest and the largest denormal, the smallest normal, ordinary values of a traversal, values far
// above every thc (t0 == t1 after rounding), FLT_MAX and +-inf. Per x also -thc (t0 = 0) and thc * +-2^24, +-2^25
// (tca +- thc round together, or differ by one ulp).
static const float TCAS[] = { 0.0f,      -0.0f,    0x1p-149f, -0x1p-149f, 0x1.fffffcp-127f, 0x1p-126f, 1.0f,
                              -1.0f,     3.7f,     0x1p-30f,  1000.0f,    0x1p40f,          0x1p100f,  -0x1p100f,
                              0x1.fffffep127f,     (float)INFINITY,       -(float)INFINITY };
#define NTCA ((int)(sizeof TCAS / sizeof TCAS[0]))

typedef struct {
    uint64_t lo, hi;
    uint64_t n_dom, bad_sel, bad_rn, n_roots, bad_roots, n_t0;
} Job;

#define CHUNK 4096u

static void* run(void* p)
{
    Job* j = (Job*)p;
    // (a chunk at a time, one simple loop per estimate and per tca: loops the compiler vectorises; a pattern outside
    // the domain is replaced by 1.0f and masked out of every count)
    static const float MULS[5] = { -1.0f, 0x1p24f, 0x1p25f, -0x1p24f, -0x1p25f };
    float xs[CHUNK], ref[CHUNK];
    uint32_t in[CHUNK];
    for (uint64_t base = j->lo; base < j->hi; base += CHUNK) {
        uint32_t n_dom = 0, bad_sel = 0, bad_rn = 0, bad_roots = 0, n_t0 = 0;
        for (uint32_t k = 0; k < CHUNK; ++k) {
            const float x = sf_rf_float((uint32_t)base + k);
            in[k] = x >= SF_ROOT_BIG_LO && x <= 0x1.fffffep127f;
            xs[k] = in[k] ? x : 1.0f;
            ref[k] = sqrtf(xs[k]);
            n_dom += in[k];
        }
        for (int e = -1; e <= 1; ++e)
            for (uint32_t k = 0; k < CHUNK; ++k) {
                const float s0 = sf_rf_float(sf_rf_bits(ref[k]) + (uint32_t)e);
                const uint32_t got = sf_rf_bits(sqrt_fix(s0, xs[k]));
                bad_sel += in[k] & (got != sf_rf_bits(sqrt_select(s0, xs[k])));
                bad_rn += in[k] & (got != sf_rf_bits(ref[k]));
            }
        for (int t = 0; t < NTCA + 5; ++t) {
            const float add = t < NTCA ? TCAS[t] : 0.0f, mul = t < NTCA ? 0.0f : MULS[t - NTCA];
            for (uint32_t k = 0; k < CHUNK; ++k) {
                const float tca = t < NTCA ? add : ref[k] * mul;
                bad_roots += in[k] & (sf_rf_bits(near_root_of(tca, ref[k])) != sf_rf_bits(root_select(tca, ref[k])));
                n_t0 += in[k] & ((tca + ref[k]) <= (tca - ref[k]));
            }
        }
        j->n_dom += n_dom, j->bad_sel += bad_sel, j->bad_rn += bad_rn;
        j->n_roots += (uint64_t)n_dom * (NTCA + 5), j->bad_roots += bad_roots, j->n_t0 += n_t0;
    }
    return NULL;
}

int main(int argc, char** argv)
{
    int nt = argc > 1 ? atoi(argv[1]) : 1;
    if (nt < 1) nt = 1;
    if (nt > 256) nt = 256;
    pthread_t th[256];
    static Job jobs[256];
    const uint64_t total = 1ull << 32, chunks = total / CHUNK;
    for (int i = 0; i < nt; ++i) {
        jobs[i].lo = chunks * (uint64_t)i / (uint64_t)nt * CHUNK;
        jobs[i].hi = chunks * (uint64_t)(i + 1) / (uint64_t)nt * CHUNK;
        if (pthread_create(&th[i], NULL, run, &jobs[i]) != 0) return 2;
    }
    Job s = { 0 };
    for (int i = 0; i < nt; ++i) {
        pthread_join(th[i], NULL);
        s.n_dom += jobs[i].n_dom, s.bad_sel += jobs[i].bad_sel, s.bad_rn += jobs[i].bad_rn;
        s.n_roots += jobs[i].n_roots, s.bad_roots += jobs[i].bad_roots, s.n_t0 += jobs[i].n_t0;
    }
    printf("%llu %llu %llu %llu %llu %llu\n", (unsigned long long)s.n_dom, (unsigned long long)s.bad_sel,
           (unsigned long long)s.bad_rn, (unsigned long long)s.n_roots, (unsigned long long)s.bad_roots,
           (unsigned long long)s.n_t0);
    return 0;
}
