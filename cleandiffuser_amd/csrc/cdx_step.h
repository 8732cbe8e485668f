// cdx_step.h -- one cdx_step record applied to one element of the state: the only copy of the solver arithmetic in device code.
//
// solver_step_kernel (cdx_bigbatch.hip), the in-LDS step of cdx_unet2_kernel, cdx_rollout_fwd_kernel and cdx_energy_kernel all call
// cdx_step_element(); what differs between them -- where the state, the bounds, the noise and the multistep / EDM memory live -- stays
// in the caller, behind a small accessor object `io`:
//     bool  has_min(), has_max(), has_mask()      is there a lower bound / an upper bound / a fix-mask
//     float x_min(), x_max(), mask(), prior()     this element's (only called where the matching has_*() holds; prior: has_mask())
//     float noise(int idx)                        this element of draw `idx` (only called with idx >= 0)
//     float prev()                                multistep memory (kind 2, vsel 2 / 3) or the EDM slope (kind 6)
//     float xold()                                EDM Heun: the state before the predictor (kind 6)
//     void  push(float v)                         remember x_theta / eps for the next multistep update
//     void  push_edm(float slope, float x)        EDM Euler: remember the slope and the state
// Every accessor is lazy: the loads are conditional and the pointers behind them may be NULL.
// The caller has already applied the classifier-free combine and the classifier-gradient shift to `p`.  EDM == false compiles kinds
// 5-7 out (the record's kind is then 0-4 by the entry point's validation).  Returns the new state after the final fix-mask blend.
#ifndef CDX_STEP_H_
#define CDX_STEP_H_

#include <hip/hip_runtime.h>

#include "../../include/cdx.h"

template <bool EDM, class IO>
__device__ __forceinline__ float cdx_step_element(const cdx_step& st, int predict_noise, float x, float p, const IO& io) {
    const float al = st.alpha, sg = st.sigma;
    const float k0 = st.k[0], k1 = st.k[1], k2 = st.k[2], k3 = st.k[3], k4 = st.k[4];
    float xn;
    if (EDM && st.kind >= 5) {  // EDM (reference newedm.py:387-401, legacy edm.py:118-160): p is the raw network output F
        float d = k0 * x + k1 * p;
        if (io.has_min()) d = fmaxf(d, io.x_min());
        if (io.has_max()) d = fminf(d, io.x_max());
        if (st.kind == 7) {  // consistency model (consistency_model.py:412-427): x <- f(x) [mask], then re-noise for the next level
            xn = d;
            if (io.has_mask()) {
                const float m = io.mask();
                xn = xn * (1.0f - m) + io.prior() * m;
            }
            if (st.noise_idx >= 0) xn += k3 * io.noise(st.noise_idx);
            return xn;
        }
        float s = (x - d) / k2;
        if (st.flags & CDX_STEP_MASK_PRED) s *= 1.0f - (io.has_mask() ? io.mask() : 0.f);   // legacy EDM masks its slope (edm.py dot_x)
        if (st.kind == 5) {
            xn = x - s * k3;
            if (st.push) io.push_edm(s, x);
        } else {
            xn = io.xold() - (io.prev() + s) / 2.0f * k3;
        }
    } else {
        if (predict_noise) {
            if (io.has_max()) p = fmaxf(p, (x - al * io.x_max()) / sg);
            if (io.has_min()) p = fminf(p, (x - al * io.x_min()) / sg);
        } else {
            if (io.has_min()) p = fmaxf(p, io.x_min());
            if (io.has_max()) p = fminf(p, io.x_max());
        }
        float eps, xth;
        if (predict_noise) { eps = p; xth = (x - sg * p) / al; }
        else { xth = p; eps = (x - al * p) / sg; }
        if (st.kind >= 3) {  // legacy DDPM class (reference diffusion/ddpm.py:153-164, 230-241): fix-mask on the prediction
            const float m = io.has_mask() ? io.mask() : 0.f;
            if (st.kind == 3) { p = p * (1.0f - m); xn = k0 * (x - k1 * p); }
            else { p = p * (1.0f - m) + x * m; xn = k0 * (k1 * x + k2 * p); }
            if (st.noise_idx >= 0) xn += k3 * io.noise(st.noise_idx);
        } else if (st.kind == 0) {
            xn = k0 * (x - k1 * eps) + k2 * eps;
            if (st.noise_idx >= 0) xn += k3 * io.noise(st.noise_idx);
        } else if (st.kind == 1) {
            xn = k0 * ((x - k1 * eps) / k2) + k3 * eps;
        } else {
            if (st.flags & CDX_STEP_MASK_PRED) {  // legacy DPMSolver (dpmsolver.py:257-264)
                const float m = io.has_mask() ? io.mask() : 0.f;
                eps = eps * (1.0f - m);
                xth = xth * (1.0f - m) + x * m;
            }
            float v = (st.vsel & 1) ? xth : eps;
            if (st.vsel == 2) v = k3 * xth - k4 * io.prev();
            if (st.vsel == 3) v = k3 * eps - k4 * io.prev();
            xn = k0 * x - k1 * v;
            if (st.noise_idx >= 0) xn += k2 * io.noise(st.noise_idx);
        }
        if (st.push) io.push(st.push == 2 ? eps : xth);
    }
    if (io.has_mask()) {
        const float m = io.mask();
        xn = xn * (1.0f - m) + io.prior() * m;
    }
    return xn;
}

#endif  // CDX_STEP_H_
