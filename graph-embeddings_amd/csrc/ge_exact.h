// ge_exact.h -- ONE update of the bit-exact trainer, shared by the two kernels that walk nonzeros sequentially inside a
// wavefront: k_adagrad_exact (glove.hip, one wave per job) and k_adagrad_strata (strata.hip, one wave per tile).
// Compile with -ffp-contract=off: Java never fuses a*b+c.
#pragma once
#include "ge_common.h"
#include "ge_cost.h"

namespace ge {

// The tables and constants exact_update reads, as a kernel argument of its own (k_adagrad_strata); k_adagrad_exact passes its
// GloveParams, which carries the same members.  Focus-side pointers are rebased so that they index by global row id.
struct ExactParams {
    float *focus, *context, *fbias, *cbias;
    float *gsf, *gsc, *gsfb, *gscb;          // Adagrad.gradSq* | Adam/AMSGrad.M1*
    float *m2f, *m2c, *m2fb, *m2cb;          // Adam/AMSGrad.M2*
    double correction;                       // Adam.java:84, per epoch
    double xmax;
    int32_t opt, D, cost_kind;
    float lr;
};

// The body of Adagrad.createJob's loop (J/opt/grad/Adagrad.java:60-95; Adam.java:103-145, AMSGrad.java:117-160) for nonzero
// (bu, bv, x), run by the 64 lanes of one wavefront-sized workgroup: products in fp32, summed sequentially in ascending d
// (GloveCost.java:10-11), fp64 sqrt/div in the update (Adagrad.java:76-77,88-89), the job's fp32 cost accumulator (:60).
// s_prod: dim floats of LDS.  Ends with a barrier: the next nonzero may read what this one wrote (same wave, program order).
template <typename P>
__device__ __forceinline__ void exact_update(const P &p, int32_t bu, int32_t bv, float x, float *s_prod, int lane, float &cost) {
    const int32_t D = p.D;
    const double lr = (double)p.lr;
    float *foc = p.focus + (int64_t)bu * D, *ctx = p.context + (int64_t)bv * D;
    float *g1s = p.gsf + (int64_t)bu * D,   *g2s = p.gsc + (int64_t)bv * D;
    for (int32_t d = lane; d < D; d += 64) s_prod[d] = foc[d] * ctx[d];
    __syncthreads();
    float ic = 0.0f;
    for (int32_t d = 0; d < D; ++d) ic = ic + s_prod[d];
    double l; float w;
    cost_terms<true>(p.cost_kind, x, p.xmax, l, w);
    ic = (float)((double)ic + ((double)(p.fbias[bu] + p.cbias[bv]) - l));
    float wc = w * ic;
    cost = (float)((double)cost + (0.5 * (double)wc) * (double)ic);
    __syncthreads();
    if (p.opt == GE_OPT_ADAGRAD) {
        for (int32_t d = lane; d < D; d += 64) {
            const float f = foc[d], c = ctx[d];
            const float grad1 = wc * c;
            const float grad2 = wc * f;
            foc[d] = (float)((double)f - ((double)grad1 / sqrt((double)g1s[d])) * lr);
            ctx[d] = (float)((double)c - ((double)grad2 / sqrt((double)g2s[d])) * lr);
            g1s[d] = g1s[d] + grad1 * grad1;
            g2s[d] = g2s[d] + grad2 * grad2;
        }
        if (lane == 0) {
            p.fbias[bu] = (float)((double)p.fbias[bu] - (double)wc / sqrt((double)p.gsfb[bu]));
            p.cbias[bv] = (float)((double)p.cbias[bv] - (double)wc / sqrt((double)p.gscb[bv]));
            wc = wc * wc;
            p.gsfb[bu] = p.gsfb[bu] + wc;
            p.gscb[bv] = p.gscb[bv] + wc;
        }
    } else {
        // Adam.java:103-145 / AMSGrad.java:117-160.  All moment arithmetic is fp32 (beta1, 1-beta1, ... are floats),
        // the parameter step goes through fp64 exactly as `focus[d1] -= correction * m1 / (sqrt(v1) + epsilon)`.
        const bool ams = p.opt == GE_OPT_AMSGRAD;
        const float beta1 = 0.9f, beta2 = 0.999f, epsilon = 1e-7f;
        const float omb1 = 1 - beta1, omb2 = 1 - beta2;
        float *m2f = p.m2f + (int64_t)bu * D, *m2c = p.m2c + (int64_t)bv * D;
        auto fmaxj = [](float a, float b) { return (a <= b) ? b : ((a + b) != (a + b) ? __builtin_nanf("") : a); };   // FastMath.max
        auto step = [&](float par, float m, float v) -> float {
            return ams ? (float)((double)par - lr / (sqrt((double)v) + (double)epsilon) * (double)m)
                       : (float)((double)par - p.correction * (double)m / (sqrt((double)v) + (double)epsilon));
        };
        for (int32_t d = lane; d < D; d += 64) {
            const float f = foc[d], c = ctx[d];
            const float grad_u = wc * c, grad_v = wc * f;
            const float m1 = beta1 * g1s[d] + omb1 * grad_u;
            const float m2 = beta1 * g2s[d] + omb1 * grad_v;
            float v1 = beta2 * m2f[d] + omb2 * (grad_u * grad_u);
            float v2 = beta2 * m2c[d] + omb2 * (grad_v * grad_v);
            if (ams) { v1 = fmaxj(m2f[d], v1); v2 = fmaxj(m2c[d], v2); }
            foc[d] = step(f, m1, v1);
            ctx[d] = step(c, m2, v2);
            g1s[d] = m1; g2s[d] = m2; m2f[d] = v1; m2c[d] = v2;
        }
        if (lane == 0) {
            const float m1 = beta1 * p.gsfb[bu] + omb1 * wc;
            const float m2 = beta1 * p.gscb[bv] + omb1 * wc;
            float v1 = beta2 * p.m2fb[bu] + omb2 * (wc * wc);
            float v2 = beta2 * p.m2cb[bv] + omb2 * (wc * wc);
            if (ams) { v1 = fmaxj(p.m2fb[bu], v1); v2 = fmaxj(p.m2cb[bv], v2); }
            p.fbias[bu] = step(p.fbias[bu], m1, v1);
            p.cbias[bv] = step(p.cbias[bv], m2, v2);
            p.gsfb[bu] = m1; p.gscb[bv] = m2; p.m2fb[bu] = v1; p.m2cb[bv] = v2;
        }
    }
    __syncthreads();   // the next nonzero may read what this one wrote (same wave, program order)
}

// Keyed bijection of [0, 2^b) (odd multiply, xor-shift, add key: each step invertible); callers cycle-walk it into [0, n).
__host__ __device__ __forceinline__ uint32_t bij_mix(uint32_t x, uint32_t m, uint32_t s, const uint32_t key[4]) {
    x = (x + key[0]) & m;  x = (x * 0x9E3779B1u) & m;  x ^= x >> s;
    x = (x + key[1]) & m;  x = (x * 0x85EBCA6Bu) & m;  x ^= x >> s;
    x = (x + key[2]) & m;  x = (x * 0xC2B2AE35u) & m;  x ^= x >> s;
    x = (x + key[3]) & m;  x = (x * 0x27D4EB2Fu) & m;  x ^= x >> s;
    return x;
}

}  // namespace ge
