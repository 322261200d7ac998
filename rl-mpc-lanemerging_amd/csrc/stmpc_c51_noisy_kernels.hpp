// stmpc_c51_noisy_kernels.hpp -- factorised-Gaussian noise on the OUTPUT layer of the C51 learner's network, plain or dueling: the sixth piece of the
// reference's third agent (rainbow.py: the `all` library's rainbow preset), after Fortunato et al. 2018, "Noisy Networks for Exploration", section 3
// (b), and Hessel et al. 2018, "Rainbow", section "Noisy Nets".  With n_out = (A + dueling) K rows and h1 inputs
//   W_eff[n][k] = mu_W[n][k] + sigma_W[n][k] f(e_out[n]) f(e_in[k]),   b_eff[n] = mu_b[n] + sigma_b[n] f(e_out[n]),   f(x) = sign(x) sqrt|x|
// with e ~ N(0, 1), h1 + n_out of them per draw.  The learner's own parameters ARE mu: nothing that reads them changes.  It restates the published
// layer; parity with the `all` library's own is not pinned (the library is absent from the reference checkout).
//
// A SHADOW network carries the noise through the kernels as they are.  The learner owns a second parameter array per draw (the DDPG layout, of which
// the b0 | W1 | b1 regions are written here) and a second packed copy of W1; the host hands k_c51_fwd (k_c51_fwd_duel), k_c51_wgrad and k_c51_act the
// learner's own C51Dev with dq.base.q.w / wt / p1 / t1 pointing at them.  What those kernels read of a network -- p0 / t0 (W0 is not noisy: shared),
// w + b0, w + W1 (the dZ1 loop), w + b1, p1 / t1 -- is then the effective network's, and net.g receives the gradient with respect to the effective
// parameters, which IS mu's gradient (dW_eff / dmu = 1).  Ring, counters, tickets and workspace are shared.  None of those kernels is edited.
//
// One noisy update is four launches (six with prioritised replay):
//   k_c51_noisy_compose   draws the noise of the online and the target net and writes their effective b0 | W1 | b1, row-major and packed, and the f
//                         vectors.  Key: dg_hash(seed ^ stream, draw, index) through dg_gauss; index k < h1 for e_in, h1 + n for e_out; the learning
//                         stream's draw is 2 * updates + net (0 online, 1 target: independent, as in Rainbow), the acting stream's a counter of its
//                         own (cnt[C51_NOISY_DRAWS]).  f goes through fp64 and is rounded to float32 once; W_eff = (float)(mu + sigma * (f_out * f_in))
//                         in fp64 with every operation explicitly unfused: one rounding (f_out * f_in is exact there).  Pad rows and columns: sigma
//                         and mu are exact zeros there and f is taken as 0, so they stay exact zeros
//   k_c51_fwd / _duel, k_c51_wgrad   on the shadow struct
//   k_c51_noisy_adam      g_sigma_W = (g_W * f_out) * f_in, g_sigma_b = g_b * f_out (float32) from net.g and the stored f of the online draw;
//                         ddpg_adam_step's arithmetic on sigma with moments of its own and mu's beta powers; sigma_target <- sigma on the updates
//                         where the hard copy runs; then dqn_adam_body on mu.  Every workgroup reads the counter and the beta powers and finishes its
//                         sigma elements BEFORE dqn_adam_body takes the ticket behind which the last workgroup advances them
// Noisy acting is k_c51_noisy_compose in acting mode (online net only, a third set of buffers, so that a learning draw survives an evaluation) and
// k_c51_act on that shadow struct.
#pragma once
#include "stmpc_c51_kernels.hpp"
#include "stmpc_c51_pop_kernels.hpp"

namespace stmpc {

constexpr int C51_NOISY_DRAWS = 5;      // the counters' slot of the acting draws (DG_CURSOR ... DG_FRAMES are 0 ... 4)
constexpr unsigned long long C51_NOISY_LEARN_STREAM = 0x6E7A6C726Eull;      // the learning draws' seed is seed ^ this ("nzlrn")
constexpr unsigned long long C51_NOISY_ACT_STREAM = 0x6E7A616374ull;        // the acting draws' ("nzact")
enum { C51_NZ_ONLINE = 0, C51_NZ_TARGET = 1, C51_NZ_ACT = 2, C51_NZ_SETS = 3 };

struct C51NoisyDev {
    float *sig, *sigt, *sm, *sv;        // sigma, the target's, Adam's moments: W1-shaped [Ap][h1p] | [Ap], padded like the parameter layout's W1 | b1
    float *f;                           // [C51_NZ_SETS][h1p + Ap]: f(e_in) [h1p] | f(e_out) [Ap] of the last online, target and acting draw
    float *we0, *we1, *we2;             // the effective parameter arrays of the three (DDPG layout; b0 | W1 | b1 written)
    float *pe0, *pe1, *pe2;             // their W1 packed for the MFMA loops
};

// f(e) of the draw's index-th variate: float32 Gaussian -> fp64 -> sign(e) sqrt|e| -> float32, one rounding (fp64's sqrt is correctly rounded)
__device__ __forceinline__ float c51_noisy_f(unsigned long long key, unsigned long long draw, int index) {
    unsigned int u1, u2;
    const double e = (double)dg_gauss(dg_hash(key, draw, (unsigned long long)index), u1, u2);
    return (float)copysign(sqrt(fabs(e)), e);
}

// mode 0: the learning draw of the current update index, online and target net (gated like the update's other kernels); mode 1: an acting draw,
// online net, and the last workgroup advances the acting-draw counter
__device__ __forceinline__ void c51_noisy_compose_body(const C51Dev &D, const C51NoisyDev &Z, int mode, int gate) {
    const DdpgDev &L = D.dq.base;
    if (mode == 0 && !ddpg_gate(L, gate)) return;
    const DdpgNet &net = L.q;
    const int h1p = L.h1p, Ap = D.dq.Ap, h1 = L.h1, n_out = L.h2;
    const int ob0 = dg_o_b0(h1p), ow1 = dg_o_w1(h1p), ob1 = dg_o_b1(h1p, Ap), nw = Ap * h1p, total = h1p + nw + Ap;
    const unsigned long long key = L.seed ^ (mode ? C51_NOISY_ACT_STREAM : C51_NOISY_LEARN_STREAM);
    const long long draws = L.cnt[C51_NOISY_DRAWS];
    const unsigned long long draw0 = mode ? (unsigned long long)draws : 2ull * (unsigned long long)L.cnt[DG_UPDATES];
    for (int set = mode ? C51_NZ_ACT : C51_NZ_ONLINE; set < (mode ? C51_NZ_SETS : C51_NZ_ACT); ++set) {
        const bool tgt = set == C51_NZ_TARGET;
        const float *mu = tgt ? net.wt : net.w, *sg = tgt ? Z.sigt : Z.sig;
        float *we = set == C51_NZ_ONLINE ? Z.we0 : (tgt ? Z.we1 : Z.we2), *pe = set == C51_NZ_ONLINE ? Z.pe0 : (tgt ? Z.pe1 : Z.pe2);
        float *f = Z.f + (size_t)set * (h1p + Ap);
        const unsigned long long draw = mode ? draw0 : draw0 + (unsigned long long)set;
        for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < total; x += gridDim.x * blockDim.x) {
            if (x < h1p) {                                          // b0 (not noisy) and f(e_in)
                we[ob0 + x] = mu[ob0 + x];
                f[x] = x < h1 ? c51_noisy_f(key, draw, x) : 0.f;
                continue;
            }
            const int j = x - h1p, n = j < nw ? j / h1p : j - nw;
            const float fo = n < n_out ? c51_noisy_f(key, draw, h1 + n) : 0.f;
            if (j < nw) {
                const int k = j % h1p;
                const float fi = k < h1 ? c51_noisy_f(key, draw, k) : 0.f;
                const float w = (float)__dadd_rn((double)mu[ow1 + j], __dmul_rn((double)sg[j], __dmul_rn((double)fo, (double)fi)));
                we[ow1 + j] = w;
                pe[dg_packed_index(n, k, h1p >> 4)] = w;            // (ddpg_repack's place for W1[n][k])
            } else {
                we[ob1 + n] = (float)__dadd_rn((double)mu[ob1 + n], __dmul_rn((double)sg[j], (double)fo));
                f[h1p + n] = fo;
            }
        }
    }
    if (!mode) return;
    __syncthreads();
    if (threadIdx.x == 0 && dg_last_block(L.tick + DG_T_ADAM, gridDim.x)) L.cnt[C51_NOISY_DRAWS] = draws + 1;      // (DG_T_ADAM: free on a discrete learner, whose Adam takes DG_T_ADAM + 1)
}
__global__ void __launch_bounds__(256) k_c51_noisy_compose(C51Dev D, C51NoisyDev Z, int mode, int gate) { c51_noisy_compose_body(D, Z, mode, gate); }

// sigma's Adam step from the effective parameters' gradient and the online draw's f, the hard copy of sigma's target, then mu's own step (D: the
// learner's own struct, not the shadow: dqn_adam_body steps and re-packs mu)
__device__ __forceinline__ void c51_noisy_adam_body(const C51Dev &D, const C51NoisyDev &Z, float lr, int gate) {
    const DdpgDev &L = D.dq.base;
    if (!ddpg_gate(L, gate)) return;
    const DdpgNet &net = L.q;
    const int h1p = L.h1p, Ap = D.dq.Ap, ow1 = dg_o_w1(h1p), nw = Ap * h1p, ns = nw + Ap;
    const float pw1 = net.bpow[0] * L.beta1, pw2 = net.bpow[1] * L.beta2;
    const bool sync = (L.cnt[DG_UPDATES] + 1) % D.dq.target_period == 0;
    const float step = lr / (1.0f - pw1), bc2s = sqrtf(1.0f - pw2);
    const float *f = Z.f;                                           // (the online draw's)
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < ns; j += gridDim.x * blockDim.x) {
        const int n = j < nw ? j / h1p : j - nw;
        const float gw = net.g[ow1 + j], fo = f[h1p + n];
        const float g = j < nw ? (gw * fo) * f[j % h1p] : gw * fo;
        const float m = L.beta1 * Z.sm[j] + L.omb1 * g;             // (ddpg_adam_step's arithmetic)
        const float v = L.beta2 * Z.sv[j] + L.omb2 * (g * g);
        const float denom = sqrtf(v) / bc2s + L.eps;
        const float s = Z.sig[j] - step * (m / denom);
        Z.sm[j] = m; Z.sv[j] = v; Z.sig[j] = s;
        if (sync) Z.sigt[j] = s;
    }
    dqn_adam_body(D.dq, lr, 0, gate);
}
__global__ void __launch_bounds__(256) k_c51_noisy_adam(C51Dev D, C51NoisyDev Z, float lr, int gate) { c51_noisy_adam_body(D, Z, lr, gate); }

// ---- a population: the two bodies on the member blockIdx.y selects from the table of the members' own structs and the table of their noise structs
// (stmpc_c51_pop_kernels.hpp's scheme: gridDim.x is the per-member block count, each member has its own tickets and counters, nothing crosses
// members).  The pass, the weight gradients and acting are k_c51_fwd_pop / k_c51_fwd_duel_pop, k_c51_wgrad_pop and k_c51_act_pop on a table of the
// members' shadow structs ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_c51_noisy_compose_pop(const C51Dev *__restrict__ members, const C51NoisyDev *__restrict__ noise, int mode, int gate) {
    const C51Dev D = members[blockIdx.y];
    c51_noisy_compose_body(D, noise[blockIdx.y], mode, gate);       // (the noise struct is read in place: a local copy of it went to scratch)
}
__global__ void __launch_bounds__(256) k_c51_noisy_adam_pop(const C51Dev *__restrict__ members, const C51NoisyDev *__restrict__ noise, DdpgLr lrs, int gate) {
    const C51Dev D = members[blockIdx.y];
    const C51NoisyDev Z = noise[blockIdx.y];
    c51_noisy_adam_body(D, Z, lrs.lr[blockIdx.y], gate);
}

}  // namespace stmpc
