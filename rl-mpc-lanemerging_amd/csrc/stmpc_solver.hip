// stmpc_solver.hip -- the batched ST solver: parameter conversion, guide tables, the launch plan's execution (solve_device) and the solve, grid,
// prediction and probe entries.  The only unit that instantiates k_solve and k_predict, lone and grouped; stmpc.hip holds the rest of the C-ABI.
#define STMPC_UNIT_SOLVER
#include "stmpc_host.hpp"
#include "stmpc_solver_groups_kernels.hpp"

namespace {
// divc<true> needs RN(1/d) to be usable by Markstein's theorem: excludes divisors whose significand is all ones
bool fastdiv_ok(double d) {
    uint64_t b; memcpy(&b, &d, 8);
    return (d > 1e-100 && d < 1e100) && ((b & 0xFFFFFFFFFFFFFull) != 0xFFFFFFFFFFFFFull);
}

// Two-operation division by d (divk in stmpc_kernels.hpp): true, with *zl = RN(1/d - RN(1/d)), if fma(x, zh, x*zl) == x/d for
// EVERY double x whose quotient neither overflows nor falls into the subnormals.  The sequence can only round wrongly when x/d
// lies within 2^-52 ulp of a midpoint, i.e. |2^t X - (2M+1) D| < 8 D 2^-52 (four-fold safety) for the significands X of x and D of d
// (odd part, L bits), t in {L-1, L, L+1}: each residue r has at most a few X in [2^52, 2^53).  All of them, their neighbours, both
// signs and three binades are run through the real arithmetic here (the CPU's fma and division are IEEE like the GPU's).
// tests/div2_check.py replays the argument exhaustively in 8-10 bit formats.
bool fastdiv2_ok(double d, double *zl_out) {
    if (!(d > 1e-100 && d < 1e100)) return false;
    const double zh = 1.0 / d;
    const double zl = std::fma(-d, zh, 1.0) / d;
    *zl_out = zl;
    int e2;
    const double m = std::frexp(d, &e2);
    uint64_t D = (uint64_t)std::ldexp(m, 53);
    while ((D & 1) == 0) D >>= 1;
    auto two = [&](double x) { volatile double u1 = x * zl; return std::fma(x, zh, (double)u1); };
    auto good = [&](double x) { return two(x) == x / d && two(-x) == -x / d; };
    if (D > 1) {
        int L = 0; while ((D >> L) != 0) ++L;
        const long long R = (long long)(((unsigned __int128)D * 8) >> 52) + 1;
        for (int t = L - 1; t <= L + 1; ++t) {
            // 2^t mod D, then its inverse (extended Euclid)
            unsigned __int128 pw = 1; for (int k = 0; k < t; ++k) pw = (pw * 2) % D;
            long long a0 = (long long)D, a1 = (long long)(uint64_t)pw, x0 = 0, x1 = 1;
            while (a1 != 0) { const long long q = a0 / a1, a2 = a0 - q * a1, x2 = x0 - q * x1; a0 = a1; a1 = a2; x0 = x1; x1 = x2; }
            if (a0 != 1) return false;                               // (cannot happen: D is odd)
            const uint64_t inv = (uint64_t)((x0 % (long long)D + (long long)D) % (long long)D);
            for (long long r = -R; r <= R; ++r) {
                if (r == 0) continue;
                const uint64_t rm = (uint64_t)(((r % (long long)D) + (long long)D) % (long long)D);
                uint64_t X = (uint64_t)(((unsigned __int128)rm * inv) % D);
                const uint64_t lo = 1ull << 52, hi = 1ull << 53;
                if (X < lo) X += ((lo - X + D - 1) / D) * D;
                int n = 0;
                for (; X < hi; X += D) {
                    if (++n > 4096) return false;                    // too many close calls to try: use ordinary division
                    for (int dx = -1; dx <= 1; ++dx) {
                        const double xb = (double)(X + dx);
                        if (!good(xb) || !good(std::ldexp(xb, -40)) || !good(std::ldexp(xb, 30))) return false;
                    }
                }
            }
        }
    }
    // (not part of the argument: a smoke test of the arithmetic on ordinary values)
    uint64_t st_ = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 4096; ++k) {
        st_ ^= st_ << 13; st_ ^= st_ >> 7; st_ ^= st_ << 17;
        const double x = (double)(st_ >> 11) * (1.0 / 9007199254740992.0) * 2.0e4 - 1.0e4;
        if (two(x) != x / d) return false;
    }
    return true;
}
}  // namespace

// np.arange(0, future_t + dt, dt) as numpy fills it (st.py:32)
void host_t_values(const stmpc_params *p, int H, double *t) {
    if (H > 0) t[0] = 0.0;
    if (H > 1) t[1] = 0.0 + p->dt;
    if (H > 2) { double d = t[1] - t[0]; for (int i = 2; i < H; ++i) t[i] = 0.0 + (double)i * d; }
}

namespace {
// Largest double q >= 0 with RN(sqrt(q)) <= m (-1 if there is none), and smallest double q >= 0 with RN(sqrt(q)) >= m (+inf if none).
// sqrt is correctly rounded on the host and on the device and monotone, so bisection over the bit patterns of the non-negative doubles is exact.
double (*volatile host_sqrt)(double) = sqrt;
double q_largest_sqrt_le(double m) {
    if (!(m >= 0.0)) return -1.0;
    uint64_t lo = 0, hi = 0x7FF0000000000000ull;            // invariant: sqrt(lo) <= m; answer in [lo, hi]
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        double q; memcpy(&q, &mid, 8);
        if (host_sqrt(q) <= m) lo = mid; else hi = mid - 1;
    }
    double q; memcpy(&q, &lo, 8);
    return q;
}
double q_smallest_sqrt_ge(double m) {
    if (!(m > 0.0)) return 0.0;                               // sqrt(0) = 0 >= m
    uint64_t lo = 0, hi = 0x7FF0000000000000ull;            // invariant: sqrt(hi) >= m (sqrt(inf) = inf)
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        double q; memcpy(&q, &mid, 8);
        if (host_sqrt(q) >= m) hi = mid; else lo = mid + 1;
    }
    double q; memcpy(&q, &hi, 8);
    return q;
}
}  // namespace

// the lattice's time layers: the range every kernel is built for, and a parameter set's count
bool bad_layers(int H) { return H < 2 || H > STMPC_H_LIMIT; }
int num_layers(const stmpc_params *p, int *H) {
    *H = stmpc_num_t(p);
    return bad_layers(*H) ? fail(STMPC_EINVAL, "number of time layers must be in [2, 64]") : STMPC_OK;
}

// How the host-pointer batch entries open: the batch's shape, the state arrays (`outs`: the entry's own required outputs are all there), each state's
// vehicle count, the context's device.  An empty batch passes untouched: the entry returns at once.
int host_batch_begin(stmpc_ctx *c, int N, int Kmax, const double *ego, const int32_t *k, const double *ox, const double *ov, bool outs) {
    TRY(check_batch(N, Kmax));
    if (N == 0) return STMPC_OK;
    if (!ego || !k || !outs) return fail(STMPC_EINVAL, "NULL host pointer");
    if (Kmax > 0 && (!ox || !ov)) return fail(STMPC_EINVAL, "NULL host pointer (other_x/other_v)");
    TRY(check_counts(N, Kmax, k));
    HIPCHK(hipSetDevice(c->device));
    return STMPC_OK;
}

int make_devp(const stmpc_params *p, DevP *d) {
    if (!p) return fail(STMPC_EINVAL, "params is NULL");
    if (!(p->ds > 0) || !(p->dt > 0)) return fail(STMPC_EINVAL, "ds and dt must be positive");
    int H;
    TRY(num_layers(p, &H));
    memset(d, 0, sizeof *d);
    d->future_s = p->future_s; d->ds = p->ds;
    double tv[STMPC_MAXH];
    host_t_values(p, H, tv);
    d->dt = tv[1] - tv[0];                       // st_cy.pyx:319 delta_t = t_indices[1] - t_indices[0]
    d->dt2 = d->dt * d->dt;                      // delta_t**2 (compiled to x*x)
    d->dt3 = host_pow(d->dt, 3.0);               // delta_t**3 -> libm pow
    d->d_w = p->d_w; d->v_w = p->v_w; d->a_w = p->a_w; d->j_w = p->j_w; d->v_des = p->v_des; d->v_max = p->v_max;
    d->a_min = p->a_min; d->a_max = p->a_max; d->j_min = p->j_min; d->j_max = p->j_max; d->min_allowed = p->min_allowed;
    d->car_length = p->car_length;
    d->obst_min_s = p->crash_min_s - p->min_allowed;
    d->max_pred_decel = p->max_pred_decel; d->follow_gap = p->follow_gap; d->react_thr = p->react_thr;
    d->crash_thr = p->crash_thr; d->crash_dist_thr = p->comb_min_dist - p->car_length;
    // (see DevP) es = +sqrt(q): es > thr <=> q > largest q with sqrt(q) <= thr; es < thr <=> q < smallest q with sqrt(q) >= thr;
    //            es = -sqrt(q): es > thr <=> sqrt(q) < -thr;                    es < thr <=> sqrt(q) > -thr
    d->q_gt_pos = q_largest_sqrt_le(p->react_thr); d->q_lt_pos = q_smallest_sqrt_ge(p->react_thr);
    d->q_gt_neg = q_smallest_sqrt_ge(-p->react_thr); d->q_lt_neg = q_largest_sqrt_le(-p->react_thr);
    d->H = H;
    d->dlen = (int)(p->car_length / p->ds);      // st.py:37
    for (int t = 0; t < H; ++t) {
        d->unc[t] = p->start_unc + p->unc_per_s * tv[t];   // st.py:40
        d->dunc[t] = (int)(d->unc[t] / p->ds);             // st.py:41
    }
    return STMPC_OK;
}

// Solver groups (main.py:43-59): the DevP of every group, after checking that the groups differ in nothing but d_w, v_w, a_w, j_w, min_allowed and
// crash_min_s.  Changes nothing; touches no device.
int check_solver_groups(const stmpc_params *groups, int G, int n_per_group, std::vector<GroupP> *out) {
    if (!groups) return fail(STMPC_EINVAL, "solver groups is NULL");
    TRY(check_group_counts(G, n_per_group, STMPC_SOLVER_GROUPS_MAX, "G must be 1 ... STMPC_SOLVER_GROUPS_MAX (512) solver groups"));
    const stmpc_params &a = groups[0];
    for (int g = 1; g < G; ++g) {
        const stmpc_params &b = groups[g];
        const Share share{"solver groups", "group", g, ": only d_w, v_w, a_w, j_w, min_allowed and crash_min_s may differ"};
        SHARED(future_s); SHARED(ds); SHARED(dt); SHARED(future_t); SHARED(start_unc); SHARED(unc_per_s); SHARED(v_des); SHARED(v_max); SHARED(a_min); SHARED(a_max);
        SHARED(j_min); SHARED(j_max); SHARED(car_length); SHARED(max_pred_decel); SHARED(follow_gap); SHARED(react_thr); SHARED(crash_thr); SHARED(comb_min_dist);
    }
    if (out) {
        out->resize((size_t)G);
        for (int g = 0; g < G; ++g) {
            GroupP &gp = (*out)[g];
            memset(&gp, 0, sizeof gp);
            if (g == 0) TRY(make_devp(&groups[0], &gp.p));
            else {
                // (the shared fields are equal, so are the values make_devp derives from them: the bisections are not repeated per group)
                gp.p = (*out)[0].p;
                gp.p.d_w = groups[g].d_w; gp.p.v_w = groups[g].v_w; gp.p.a_w = groups[g].a_w; gp.p.j_w = groups[g].j_w;
                gp.p.min_allowed = groups[g].min_allowed;
                gp.p.obst_min_s = groups[g].crash_min_s - groups[g].min_allowed;
            }
        }
    }
    return STMPC_OK;
}

namespace {
// Table of the guided bounding attempt (SolveArgs::guide_tab): the optimal step sequence of the OBSTACLE-FREE problem from every lattice state
// (i1 = cells covered in the last layer, d = i1 - cells covered in the layer before), by backward dynamic programming over the true state
// (speed, acceleration) -- not the reference's history-collapsed search, whose answer it only approximates: the table centres a search, it
// never supplies a cost.  Ranges are st_cy.pyx:65-75 in cell units, shrunk by 1e-6 cell; costs st_cy.pyx:46-50 without the gap term.
// Returns false (no table: the attempt is skipped) for parameter sets whose state space does not fit a byte per step.
bool build_guide_table(const DevP &dp, std::vector<unsigned char> &tab, int &imax_out, int &D_out) {
    const int H = dp.H;
    const double ds = dp.ds, dt = dp.dt, u = ds / dt;
    if (H < 3 || !(ds > 0) || !(dt > 0)) return false;
    const int imax = (int)floor(dp.v_max * dt / ds + 1e-9);
    const int D = (int)ceil(fmax(fabs(dp.a_min), fabs(dp.a_max)) * dt * dt / ds) + 1;
    if (imax < 1 || imax > 254 || D > 60) return false;
    const int nd = 2 * D + 1, nS = (imax + 1) * nd, R = H - 1;
    std::vector<double> Fp((size_t)nS, 0.0), Fc((size_t)nS);
    std::vector<unsigned char> pol((size_t)(R + 1) * nS, 255);
    for (int r = 1; r <= R; ++r) {
        for (int i1 = 0; i1 <= imax; ++i1) for (int dd = -D; dd <= D; ++dd) {
            const int st = i1 * nd + dd + D, i2 = i1 - dd;
            Fc[st] = INFINITY;
            if (i2 < 0 || i2 > imax) continue;
            const double v = i1 * u, pv = i2 * u, a = (v - pv) / dt;
            const double lo_a = fmax(a + dp.j_min * dt, dp.a_min), hi_a = fmin(a + dp.j_max * dt, dp.a_max);
            const double lo_v = fmax(v + lo_a * dt, 0.0), hi_v = fmin(v + hi_a * dt, dp.v_max);
            int lo = (int)ceil(lo_v * dt / ds + 1e-6), hi = (int)floor(hi_v * dt / ds - 1e-6);
            lo = lo < i1 - D ? i1 - D : lo; lo = lo < 0 ? 0 : lo;
            hi = hi > i1 + D ? i1 + D : hi; hi = hi > imax ? imax : hi;
            double best = INFINITY; int arg = 255;
            for (int i0 = lo; i0 <= hi; ++i0) {
                const double vv = i0 * u - dp.v_des, aa = (i0 - i1) * u / dt, jj = (i0 - 2 * i1 + i2) * u / (dt * dt);
                const double tot = dp.v_w * vv * vv + dp.a_w * aa * aa + dp.j_w * jj * jj + Fp[(size_t)i0 * nd + (i0 - i1 + D)];
                if (tot < best) { best = tot; arg = i0; }
            }
            Fc[st] = best; pol[(size_t)r * nS + st] = (unsigned char)arg;
        }
        Fp.swap(Fc);
    }
    tab.assign((size_t)nS * R, 255);
    for (int i1 = 0; i1 <= imax; ++i1) for (int dd = -D; dd <= D; ++dd) {
        int c1 = i1, c2 = i1 - dd;
        if (c2 < 0 || c2 > imax) continue;
        unsigned char *row = &tab[(size_t)(i1 * nd + dd + D) * R];
        for (int t = 1; t <= R; ++t) {
            const int dcur = c1 - c2;
            if (dcur < -D || dcur > D) break;
            const int i0 = pol[(size_t)(R - t + 1) * nS + c1 * nd + dcur + D];
            if (i0 == 255) break;
            row[t - 1] = (unsigned char)i0;
            c2 = c1; c1 = i0;
        }
    }
    imax_out = imax; D_out = D;
    return true;
}
// Synchronous entries that reuse the counters: an error flag raised by an earlier asynchronous solve and not yet seen by
// stmpc_get_stats / stmpc_check_error is moved to the context's sticky word first (k_predict does the same on the device).
int latch_solver_error(stmpc_ctx *c) {
    if (!c->solver.counters.p) return STMPC_OK;
    HIPCHK(hipDeviceSynchronize());
    unsigned cur = 0;
    HIPCHK(hipMemcpy(&cur, (const unsigned *)c->solver.counters.p + STMPC_CNT_ERR, sizeof cur, hipMemcpyDeviceToHost));
    if (cur) { const unsigned one = 1u; HIPCHK(hipMemcpy(c->sticky.p, &one, sizeof one, hipMemcpyHostToDevice)); }
    return STMPC_OK;
}
template <int KMAX>
void launch_predict(const DevP &dp, int N, int Kmax, const double *ego, const int *k, const double *ox, const double *ov,
                    CarTab tab, unsigned *counters, u64 *ubound, int *queue1, unsigned *proxy0, int *resume_t, unsigned char *prio_key, hipStream_t st,
                    unsigned *sticky = nullptr, const unsigned char *guide_tab = nullptr, int guide_imax = 0, int guide_D = 0, u16 *guide = nullptr) {
    constexpr int E = PredShape<KMAX>::E;          // episodes per wavefront (k_predict)
    int blocks = (N + E - 1) / E;
    hipLaunchKernelGGL(k_predict<KMAX>, dim3(blocks), dim3(128), 0, st, dp, N, Kmax, ego, k, ox, ov, tab, counters, ubound, queue1, proxy0, resume_t, prio_key, sticky,
                       guide_tab, guide_imax, guide_D, guide, 0);
}

template <int KMAX>
void launch_predict_groups(const DevP &dp, GroupTab gt, int N, int Kmax, const double *ego, const int *k, const double *ox, const double *ov,
                           CarTab tab, unsigned *counters, u64 *ubound, int *queue1, unsigned *proxy0, int *resume_t, unsigned char *prio_key, hipStream_t st,
                           unsigned *sticky, const unsigned char *guide_tab, int guide_imax, int guide_D, u16 *guide) {
    constexpr int E = PredShape<KMAX>::E;
    int blocks = (N + E - 1) / E;
    hipLaunchKernelGGL(grouped::k_predict<KMAX>, dim3(blocks), dim3(128), 0, st, dp, gt, N, Kmax, ego, k, ox, ov, tab, counters, ubound, queue1, proxy0, resume_t, prio_key,
                       sticky, guide_tab, guide_imax, guide_D, guide, 0);
}
}  // namespace

extern "C" {

int stmpc_solve_batch_device(stmpc_ctx *c, const stmpc_params *p, int N, int Kmax, const double *d_ego,
                             const int32_t *d_k, const double *d_ox, const double *d_ov, int32_t *d_path,
                             int32_t *d_bt, double *d_cost, double *d_pd, int32_t *d_crash, void *stream) {
    return stmpc_solve_batch_device_ac(c, p, N, Kmax, d_ego, d_k, d_ox, d_ov, d_path, d_bt, d_cost, d_pd, d_crash, nullptr, stream);
}

int stmpc_solve_batch_device_ac(stmpc_ctx *c, const stmpc_params *p, int N, int Kmax, const double *d_ego,
                                const int32_t *d_k, const double *d_ox, const double *d_ov, int32_t *d_path,
                                int32_t *d_bt, double *d_cost, double *d_pd, int32_t *d_crash, double *d_action_cost, void *stream) {
    return solve_device(c, p, nullptr, N, Kmax, d_ego, d_k, d_ox, d_ov, d_path, d_bt, d_cost, d_pd, d_crash, d_action_cost, stream);
}

}  // extern "C"

namespace {
// ---- one k_solve launch ------------------------------------------------------------------------------------------------------------------
struct SolveLaunch { dim3 grid, block; size_t lds; hipStream_t stream; const SolveArgs &a; const GroupTab *g; };

int no_such_variant() { return fail(STMPC_EINTERNAL, "k_solve: no such kernel variant"); }

// f(std::integral_constant of the one of Vs that x equals); refused when it equals none
template <auto... Vs, class X, class F> int with_value(X x, F &&f) {
    int rc = STMPC_OK;
    const bool found = ((x == Vs && ((rc = f(std::integral_constant<decltype(Vs), Vs>{})), true)) || ...);
    return found ? rc : no_such_variant();
}

// one instantiation: compiled when plan::variant_built lists it, refused otherwise.  Raises the kernel's dynamic LDS limit where the launch needs
// more than 48 KB, and launches it.
template <bool G, bool L, bool FD, int KT, int FM, bool SG, int RS, int NWX>
int launch_instance(const SolveLaunch &l) {
    if constexpr (!plan::variant_built(plan::KernelVariant{L, FD, KT, FM, SG, RS, NWX, G})) return no_such_variant();
    else {
        const auto launch = [&l](auto *kernel, const auto &args) -> int {
            if (l.lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds));
            hipLaunchKernelGGL(kernel, l.grid, l.block, l.lds, l.stream, args);
            return STMPC_OK;
        };
        if constexpr (G) {
            SolveArgsG ag;
            memset(&ag, 0, sizeof ag);
            static_cast<SolveArgs &>(ag) = l.a;
            ag.g = *l.g;
            return launch(grouped::k_solve<L, false, FD, KT, FM, SG, RS, NWX>, ag);
        } else return launch(k_solve<L, false, FD, KT, FM, SG, RS, NWX>, l.a);
    }
}

// The k_solve instantiation of a variant, each template argument picked from the values it takes in some instantiation.
int launch_k_solve(const plan::KernelVariant &v, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const SolveArgs &a, const GroupTab *g) {
    if (!plan::variant_built(v) || (v.grouped && !g)) return no_such_variant();
    const SolveLaunch l{grid, block, lds, stream, a, g};
    return with_value<false, true>(v.grouped, [&](auto G) { return with_value<false, true>(v.use_lds, [&](auto L) {
           return with_value<false, true>(v.fastdiv, [&](auto FD) { return with_value<0, 8>(v.kt, [&](auto KT) {
           return with_value<9, STMPC_FAN1, STMPC_FAN88>(v.fanmax, [&](auto FM) { return with_value<false, true>(v.s1gen, [&](auto SG) {
           return with_value<0, 1, 2>(v.res, [&](auto RS) { return with_value<4, STMPC_MAXWAVES, 88>(v.nwx, [&](auto NWX) {
               return launch_instance<decltype(G)::value, decltype(L)::value, decltype(FD)::value, decltype(KT)::value, decltype(FM)::value,
                                      decltype(SG)::value, decltype(RS)::value, decltype(NWX)::value>(l); }); }); }); }); }); }); }); });
}

// ---- guide tables of the guided bounding attempt (SolveArgs::guide_tab) ------------------------------------------------------------------------
struct Guide { const unsigned char *tab = nullptr; int imax = 0, D = 0; };

// One parameter set: the table depends on the dynamics and the cost weights only; rebuilt when they change (a few ms on the host)
int guide_for_params(stmpc_ctx::Solver &sv, const DevP &dp, hipStream_t st, Guide *out) {
    const double key[12] = {dp.ds, dp.dt, dp.v_w, dp.a_w, dp.j_w, dp.v_des, dp.v_max, dp.a_min, dp.a_max, dp.j_min, dp.j_max, (double)dp.H};
    stmpc_ctx::Solver::GuideSlot *slot = nullptr;
    for (auto &g : sv.guides) if (g.valid && memcmp(key, g.key, sizeof key) == 0) { slot = &g; break; }
    if (!slot) {
        // A parameter set not seen before (or replaced since): build its table on the host (a few ms) and queue the upload on THIS call's
        // stream, ahead of the kernels that read it.  Nothing waits for the device unless a table has to be replaced (a fifth parameter set):
        // kernels of earlier calls may still read the one that goes.
        for (auto &g : sv.guides) if (!g.valid) { slot = &g; break; }
        if (!slot) {
            slot = &sv.guides[0];
            for (auto &g : sv.guides) if (g.last_use < slot->last_use) slot = &g;
            slot->valid = false;
            HIPCHK(hipDeviceSynchronize());
        }
        slot->ok = build_guide_table(dp, slot->host, slot->imax, slot->D);
        if (slot->ok) {
            TRY(slot->dev.ensure(slot->host.size()));
            HIPCHK(hipMemcpyAsync(slot->dev.p, slot->host.data(), slot->host.size(), hipMemcpyHostToDevice, st));
        }
        memcpy(slot->key, key, sizeof key);
        slot->valid = true;                 // (only after the upload has been queued successfully)
    }
    slot->last_use = ++sv.guide_clock;
    if (slot->ok) *out = Guide{slot->dev.as<unsigned char>(), slot->imax, slot->D};
    return STMPC_OK;
}

// The groups' table: per group the DevP, the band of its own weights and the offset of its own guide table (one table per distinct
// (v_w, a_w, j_w), built on the host and stored one after another).  The device copies are kept while the next call brings an equal table;
// replacing them waits for the device first (kernels of earlier calls may still read them).
int guide_for_groups(stmpc_ctx::Solver &sv, const plan::SolvePlan &pl, SolverGroupsHost *sg, GroupTab *gtab, Guide *out) {
    for (auto &gp : sg->table) { plan::band_for(pl.k, gp.p, &gp.band, &gp.band2_mult); gp.guide_off = -1; }
    const bool same = sv.sg.host.size() == sg->table.size() && [&] {
        for (size_t g = 0; g < sg->table.size(); ++g) {
            GroupP x = sv.sg.host[g]; x.guide_off = -1;
            if (memcmp(&x, &sg->table[g], sizeof x) != 0) return false;
        }
        return true;
    }();
    if (!same || sv.sg.want_guide != pl.guided) {
        std::vector<unsigned char> all;
        std::vector<int> built;                          // groups whose table is in `all`
        bool ok = pl.guided;
        int imax = 0, D = 0;
        for (size_t g = 0; g < sg->table.size() && ok; ++g) {
            GroupP &gp = sg->table[g];
            for (int b : built)
                if (sg->table[b].p.v_w == gp.p.v_w && sg->table[b].p.a_w == gp.p.a_w && sg->table[b].p.j_w == gp.p.j_w) { gp.guide_off = sg->table[b].guide_off; break; }
            if (gp.guide_off >= 0) continue;
            std::vector<unsigned char> one;
            ok = build_guide_table(gp.p, one, imax, D);
            if (!ok) break;
            gp.guide_off = (long long)all.size();
            all.insert(all.end(), one.begin(), one.end());
            built.push_back((int)g);
        }
        if (!ok) for (auto &gp : sg->table) gp.guide_off = 0;
        HIPCHK(hipDeviceSynchronize());
        sv.sg.host.clear();
        TRY(upload(sv.sg.table, sg->table.data(), sg->table.size()));
        if (ok) TRY(upload(sv.sg.guide, all.data(), all.size()));
        sv.sg.want_guide = pl.guided; sv.sg.guide_ok = ok; sv.sg.guide_imax = imax; sv.sg.guide_D = D;
        sv.sg.host = sg->table;
    }
    gtab->groups = sv.sg.table.as<GroupP>(); gtab->n_per_group = sg->n_per_group;
    if (pl.guided && sv.sg.guide_ok) *out = Guide{sv.sg.guide.as<unsigned char>(), sv.sg.guide_imax, sv.sg.guide_D};
    return STMPC_OK;
}
}  // namespace

// The batched solve behind every solver entry: carries out plan::plan_solve's plan.  sg: null, or the groups of a grouped call (p is then groups[0],
// read for the shared fields): k_predict and the k_solve launches are replaced by the kernels of namespace grouped.
int solve_device(stmpc_ctx *c, const stmpc_params *p, SolverGroupsHost *sg, int N, int Kmax, const double *d_ego,
                 const int32_t *d_k, const double *d_ox, const double *d_ov, int32_t *d_path,
                 int32_t *d_bt, double *d_cost, double *d_pd, int32_t *d_crash, double *d_action_cost, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (N < 0 || Kmax < 0 || Kmax > STMPC_KMAX_LIMIT) return fail(STMPC_EINVAL, "N or Kmax out of range");
    if (N == 0) return STMPC_OK;
    if (!d_ego || !d_k || !d_path || !d_bt || !d_cost) return fail(STMPC_EINVAL, "NULL device pointer");
    if (Kmax > 0 && (!d_ox || !d_ov)) return fail(STMPC_EINVAL, "NULL device pointer (other_x/other_v)");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    stmpc_ctx::Solver &sv = c->solver;
    DevP dp;
    TRY(make_devp(p, &dp));
    const int H = dp.H;
    const int S_nom = stmpc_num_s(p, 0.0);
    if (S_nom < 2 || S_nom + 2 > STMPC_S_LIMIT) return fail(STMPC_EINVAL, "number of position cells out of range");
    // FASTDIV kernels: Markstein's five-operation quotient for the lattice step (per-episode value), the two-operation one for
    // dt, dt^2, dt^3 once each of them has passed fastdiv2_ok (cached per context: the check costs a few hundred divisions)
    if (sv.fd2_dt != dp.dt || sv.fd2_dt2 != dp.dt2 || sv.fd2_dt3 != dp.dt3) {
        sv.fd2_dt = dp.dt; sv.fd2_dt2 = dp.dt2; sv.fd2_dt3 = dp.dt3;
        sv.fd2_ok = fastdiv2_ok(dp.dt, &sv.fd2_zl[0]) && fastdiv2_ok(dp.dt2, &sv.fd2_zl[1]) && fastdiv2_ok(dp.dt3, &sv.fd2_zl[2]);
    }
    plan::SolveHistory hist;
    if (sv.h_overflow) { hist.overflow[0] = sv.h_overflow[0]; hist.overflow[1] = sv.h_overflow[1]; }
    hist.last_has_hbm = sv.last_has_hbm; hist.last_hbm_tier_count = sv.last_hbm_tier_count;
    hist.fastdiv_proven = fastdiv_ok(dp.dt) && fastdiv_ok(dp.dt2) && fastdiv_ok(dp.dt3) && sv.fd2_ok;
    const plan::SolvePlan pl = plan::plan_solve(sv.knobs, plan::DeviceShape{c->num_cu, c->lds_per_block}, dp, N, Kmax, sg != nullptr, hist);
    const int Kalloc = pl.Kalloc, nt = pl.nt;

    // scratch
    TRY(sv.tab_edge.ensure((size_t)N * H * Kalloc * 2 * sizeof(double)));
    TRY(sv.tab_win.ensure((size_t)N * H * Kalloc * 2 * sizeof(int)));
    TRY(sv.tab_nact.ensure((size_t)N * H * sizeof(int)));
    TRY(sv.tab_nums.ensure((size_t)N * sizeof(int)));
    if (!sv.counters.p) { TRY(sv.counters.ensure(64 * sizeof(unsigned))); HIPCHK(hipMemsetAsync(sv.counters.p, 0, 64 * sizeof(unsigned), st)); }
    TRY(sv.lists.ensure((size_t)STMPC_MAX_TIERS * N * sizeof(int)));
    TRY(sv.ubound.ensure((size_t)N * sizeof(u64)));
    TRY(sv.proxy.ensure((size_t)N * sizeof(unsigned)));
    TRY(sv.order.ensure((size_t)N * sizeof(int)));

    // the checkpoint pool: the plan wants it, the device's memory decides
    bool resume = pl.resume_wanted;
    if (resume && sv.pool_bp.cap + sv.ckpt.cap < pl.pool_bytes) {
        // a growing request: only while it is at most a quarter of what the device has free right now (a process shared with torch / RCCL).
        // A request that was turned down is priced again every 64th call: memory another tenant held at that moment may be free by now.
        if (sv.resume_refused_for == pl.pool_bytes && (++sv.resume_refused_calls & 63) != 0) resume = false;
        else {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
            if (pl.pool_bytes > (free_b + sv.pool_bp.cap + sv.ckpt.cap) / 4) { resume = false; sv.resume_refused_for = pl.pool_bytes; }
            else sv.resume_refused_for = 0;
        }
    }
    if (resume) {
        // if the device cannot spare it, overflowing searches restart in the wider window instead of continuing
        if (sv.pool_bp.ensure((size_t)pl.pool_cap * H * pl.tier[0].W * pl.bp_elem) || sv.ckpt.ensure((size_t)pl.pool_cap * pl.ckpt_stride) || sv.resume_t.ensure((size_t)N * sizeof(int))) {
            (void)hipGetLastError();
            sv.pool_bp.release(); sv.ckpt.release();
            resume = false;
        }
    }
    for (int k = 0; k < nt; ++k)                 // back-pointers of a tier: per resident workgroup
        TRY(sv.bp_tier[k].ensure((size_t)pl.tier[k].grid * H * pl.tier[k].W * pl.bp_elem));
    sv.last_resume_refused = pl.resume_wanted && !resume;
    int *resume_t = resume ? sv.resume_t.as<int>() : nullptr;
    if (pl.need_hbm_tier) TRY(sv.gscratch.ensure((size_t)pl.tier[nt - 1].grid * ((size_t)pl.Wg * STMPC_CELL_BYTES + STMPC_LIST_SLACK + (size_t)pl.Wg * 8)));

    CarTab tab{sv.tab_edge.as<double>(), sv.tab_win.as<int>(), sv.tab_nact.as<int>(), sv.tab_nums.as<int>()};
    unsigned *counters = sv.counters.as<unsigned>();

    hipEvent_t e0 = sv.ev0, e1 = sv.ev1, e2 = sv.ev2, e3 = sv.ev3;
    if (sv.profiling) {
        if (sv.pool_used + 4 > sv.pool.size()) {
            for (int i = 0; i < 4; ++i) { hipEvent_t ev; HIPCHK(hipEventCreate(&ev)); sv.pool.push_back(ev); }
        }
        e0 = sv.pool[sv.pool_used]; e1 = sv.pool[sv.pool_used + 1]; e2 = sv.pool[sv.pool_used + 2]; e3 = sv.pool[sv.pool_used + 3];
        sv.pool_used += 4;
    }
    if (!sv.h_overflow) {
        HIPCHK(hipHostMalloc((void **)&sv.h_overflow, 2 * sizeof(int), hipHostMallocMapped)); sv.h_overflow[0] = 0; sv.h_overflow[1] = 0;
        HIPCHK(hipHostGetDevicePointer((void **)&sv.d_overflow, sv.h_overflow, 0));
    }
    int *queue1 = pl.overlap ? sv.lists.as<int>() + (size_t)N : nullptr;
    unsigned *proxy0 = pl.split ? sv.proxy.as<unsigned>() : nullptr;
    if (pl.heavy_first) TRY(sv.prio_key.ensure((size_t)N));
    unsigned char *prio_key = pl.heavy_first ? sv.prio_key.as<unsigned char>() : nullptr;
    Guide guide;
    GroupTab gtab{nullptr, 0};
    if (sg) TRY(guide_for_groups(sv, pl, sg, &gtab, &guide));
    else if (pl.guided) TRY(guide_for_params(sv, dp, st, &guide));
    u16 *g_cells = nullptr;
    if (guide.tab) { TRY(sv.guide_cells.ensure((size_t)N * H * sizeof(u16))); g_cells = sv.guide_cells.as<u16>(); }
    HIPCHK(hipEventRecord(e0, st));
    with_kmax(Kalloc, [&](auto km) {
        if (sg) launch_predict_groups<decltype(km)::value>(dp, gtab, N, Kalloc, d_ego, d_k, d_ox, d_ov, tab, counters, sv.ubound.as<u64>(), queue1, proxy0, resume_t,
                                                           prio_key, st, c->sticky.as<unsigned>(), guide.tab, guide.imax, guide.D, g_cells);
        else launch_predict<decltype(km)::value>(dp, N, Kalloc, d_ego, d_k, d_ox, d_ov, tab, counters, sv.ubound.as<u64>(), queue1, proxy0, resume_t, prio_key, st,
                                                 c->sticky.as<unsigned>(), guide.tab, guide.imax, guide.D, g_cells);
    });

    SolveArgs a;
    memset(&a, 0, sizeof a);
    a.p = dp; a.N = N; a.Kmax = Kalloc;
    a.ego = d_ego; a.tab = tab;
    a.counters = counters; a.lists = sv.lists.as<int>(); a.ubound = sv.ubound.as<u64>();
    a.prune = pl.prune_on;
    a.band = pl.band; a.band2_mult = pl.band2_mult;
    a.band_cap = pl.k.band_cap;
    for (int i = 0; i < 3; ++i) a.retry_mult[i] = pl.k.retry_mult[i];
    a.bound_infl = pl.k.bound_infl; a.last_infl = pl.k.last_infl;
    a.guide = g_cells; a.tube_w = pl.k.tube_w; a.tube_dense = pl.k.tube_dense; a.band_dense = pl.k.band_dense;
    a.retry_move = resume ? pl.k.retry_move : 0;
    a.prio_thr = pl.k.prio_thr; a.prio_mode = pl.k.prio_mode;
    a.bp_rel8 = pl.bp_rel8 ? 1 : 0;
    a.force_general = pl.k.force_general ? 1 : 0;
    a.gsh_max = pl.k.gsh_max;
    a.zl_dt = sv.fd2_zl[0]; a.zl_dt2 = sv.fd2_zl[1]; a.zl_dt3 = sv.fd2_zl[2];
#ifdef STMPC_PHASE_PROF
    TRY(sv.phase_prof.ensure(4 * STMPC_NPH * sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(sv.phase_prof.p, 0, 4 * STMPC_NPH * sizeof(unsigned long long), st));
    a.phase_prof = sv.phase_prof.as<unsigned long long>();
#endif
    a.ckpt = resume ? sv.ckpt.as<unsigned char>() : nullptr; a.ckpt_stride = pl.ckpt_stride; a.resume_t = resume_t;
    a.pool_bp = resume ? sv.pool_bp.as<unsigned char>() : nullptr; a.pool_cap = resume ? pl.pool_cap : 0;
    a.W0 = pl.tier[0].W;
    a.maxshift = pl.maxshift;
    a.proxy = sv.proxy.as<unsigned>();
    a.path_idx = d_path; a.best_t = d_bt; a.cost = d_cost; a.path_dist = d_pd; a.crash = d_crash; a.action_cost = d_action_cost;
    a.host_overflow = sv.d_overflow;
    if (pl.retire) {
        TRY(sv.cu_tab.ensure(1025 * sizeof(unsigned)));
        HIPCHK(hipMemsetAsync(sv.cu_tab.p, 0, 1025 * sizeof(unsigned), st));
        a.cu_tab = sv.cu_tab.as<unsigned>(); a.retire_from = pl.retire_from; a.retire_left = pl.retire_left;
    }
    HIPCHK(hipEventRecord(e1, st));
    if (pl.overlap) HIPCHK(hipEventRecord(sv.ev_fork, st));      // the vehicle table and the preset queue are ready

    // the schedule, step by step: wait, launch, record
    auto stream_of = [&](plan::Stream s) { return s == plan::Stream::Side ? sv.aux_stream : s == plan::Stream::Masked ? sv.main_masked : s == plan::Stream::Reserved ? sv.aux_reserved : st; };
    auto event_of = [&](plan::Event e) { return e == plan::Event::Fork ? sv.ev_fork : e == plan::Event::Join ? sv.ev_join : e == plan::Event::Join0 ? sv.ev_join0 : e == plan::Event::JoinR ? sv.ev_join_r : e2; };
    for (int i = 0; i < pl.n_steps; ++i) {
        const plan::PlanStep &s = pl.steps[i];
        hipStream_t lst = stream_of(s.stream);
        if (s.wait != plan::Event::None) HIPCHK(hipStreamWaitEvent(lst, event_of(s.wait), 0));
        if (s.op == plan::Op::Order8) hipLaunchKernelGGL(k_order8, dim3(1), dim3(1024), 0, lst, N, (const unsigned char *)prio_key, sv.order.as<int>());
        else if (s.op == plan::Op::Order) hipLaunchKernelGGL(k_order, dim3(1), dim3(1024), 0, lst, N, (const unsigned *)sv.proxy.as<unsigned>(), sv.order.as<int>());
        else if (s.op == plan::Op::Solve) {
            // side = on the side (or reserved) stream, consuming tier 0's overflow queue while tier 0 is still running
            const plan::PlanTier &t = pl.tier[s.tier];
            const bool side = s.stream == plan::Stream::Side || s.stream == plan::Stream::Reserved;
            a.concurrent = side ? 1 : 0;
            a.always_wait = s.stream == plan::Stream::Reserved ? 1 : 0;
            a.split = (pl.split && s.tier == 0) ? 1 : 0;
            a.feeds_concurrent = (pl.overlap && s.tier == 0) ? 1 : 0;
            a.prev_grid = side ? pl.tier[0].grid : 0;
            a.wait_ticks = side ? 20000000ull : 0ull;             // 0.2 s of the 100 MHz clock
            a.phase = s.phase;
            a.order = ((s.phase == 2 || pl.heavy_first) && s.tier == 0) ? sv.order.as<int>() : nullptr;
            a.W = t.W; a.PW = t.PW; a.tier = s.tier; a.last_tier = (s.tier == nt - 1);
            a.bp = sv.bp_tier[s.tier].as<u16>();
            a.gscratch = t.lds ? nullptr : sv.gscratch.as<unsigned char>();
            TRY(launch_k_solve(resume ? t.variant_resume : t.variant, dim3(s.grid), dim3(64 * t.waves), t.lds_bytes, lst, a, sg ? &gtab : nullptr));
        }
        if (s.record != plan::Event::None) HIPCHK(hipEventRecord(event_of(s.record), lst));
    }
    HIPCHK(hipEventRecord(e3, st));
    HIPCHK(hipGetLastError());
    c->stats.episodes = N;
    sv.last_nt = nt; sv.last_has_hbm = pl.need_hbm_tier;
    c->stats_pending = !sv.profiling;
    if (sv.profiling) { sv.acc_launches += 1; sv.acc_episodes += N; }
    return STMPC_OK;
}

extern "C" {

int stmpc_get_stats(stmpc_ctx *c, stmpc_stats *out) {
    if (!c || !out) return fail(STMPC_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    if (c->stats_pending) {
        HIPCHK(hipEventSynchronize(c->solver.ev3));
        unsigned cnt[64];
        HIPCHK(hipMemcpy(cnt, c->solver.counters.p, sizeof cnt, hipMemcpyDeviceToHost));
        float ms_all = 0.f, ms_dp = 0.f;
        HIPCHK(hipEventElapsedTime(&ms_all, c->solver.ev0, c->solver.ev3));
        HIPCHK(hipEventElapsedTime(&ms_dp, c->solver.ev1, c->solver.ev2));
#ifdef STMPC_PHASE_PROF
        if (const char *f = getenv("STMPC_PHASE_DUMP")) {
            unsigned long long pp[4 * STMPC_NPH];
            HIPCHK(hipMemcpy(pp, c->solver.phase_prof.p, sizeof pp, hipMemcpyDeviceToHost));
            FILE *fp = fopen(f, "w");
            if (fp) { for (int m = 0; m < 4; ++m) { for (int k = 0; k < STMPC_NPH; ++k) fprintf(fp, "%llu ", pp[m * STMPC_NPH + k]); fprintf(fp, "\n"); } fclose(fp); }
        }
#endif
        c->stats.fallback = cnt[4];                       // episodes that overflowed the first LDS window
        c->stats.hbm_tier = (c->solver.last_has_hbm && c->solver.last_nt >= 2) ? cnt[4 * (c->solver.last_nt - 1)] : 0;
        c->stats.fast_path = c->stats.episodes - cnt[4];
        c->solver.last_hbm_tier_count = c->stats.hbm_tier;
        c->stats.resume_refused = c->solver.last_resume_refused ? 1 : 0;
        c->stats.pool_exhausted = cnt[STMPC_CNT_POOL_FULL];
        c->stats.retries = cnt[STMPC_CNT_RETRY];
        c->stats.guided = cnt[STMPC_CNT_GUIDED];
        c->stats.nodes_exact = cnt[STMPC_CNT_NODES_EXACT];
        c->stats.nodes_bound = cnt[STMPC_CNT_NODES_BOUND];
        c->stats.solve_ms = ms_all;
        c->stats.dp_kernel_ms = ms_dp;
        c->stats_pending = false;
        if (cnt[STMPC_CNT_ERR]) {
            // reported here, once: cleared so that the next k_predict does not latch it again and blame a later batch
            HIPCHK(hipMemset((unsigned *)c->solver.counters.p + STMPC_CNT_ERR, 0, sizeof(unsigned)));
            *out = c->stats;
            return fail(STMPC_EINTERNAL, "solver error flag set on device");
        }
    }
    *out = c->stats;
    return STMPC_OK;
}

int stmpc_profile(stmpc_ctx *c, int enable, stmpc_profile_totals *out) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    if (enable) {
        c->solver.profiling = true; c->solver.pool_used = 0;
        c->solver.acc_solve_ms = c->solver.acc_dp_ms = 0; c->solver.acc_launches = c->solver.acc_fallback = c->solver.acc_episodes = 0;
        return STMPC_OK;
    }
    // disable: drain the pool
    for (size_t i = 0; i + 3 < c->solver.pool_used; i += 4) {
        HIPCHK(hipEventSynchronize(c->solver.pool[i + 3]));
        float a = 0.f, b = 0.f;
        HIPCHK(hipEventElapsedTime(&a, c->solver.pool[i], c->solver.pool[i + 3]));
        HIPCHK(hipEventElapsedTime(&b, c->solver.pool[i + 1], c->solver.pool[i + 2]));
        c->solver.acc_solve_ms += a; c->solver.acc_dp_ms += b;
    }
    c->solver.pool_used = 0;
    c->solver.profiling = false;
    if (out) {
        out->launches = c->solver.acc_launches; out->episodes = c->solver.acc_episodes;
        out->solve_ms = c->solver.acc_solve_ms; out->dp_kernel_ms = c->solver.acc_dp_ms;
    }
    return STMPC_OK;
}

int stmpc_solve_batch(stmpc_ctx *c, const stmpc_params *p, int N, int Kmax, const double *ego, const int32_t *k,
                      const double *ox, const double *ov, int32_t *path, int32_t *bt, double *cost, double *pd,
                      int32_t *crash) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    TRY(host_batch_begin(c, N, Kmax, ego, k, ox, ov, path && bt && cost));
    if (N == 0) return STMPC_OK;
    int H;
    TRY(num_layers(p, &H));
    auto &s = c->s;
    const size_t n = (size_t)N;
    TRY(s.path.ensure(n * H * 4)); TRY(s.bt.ensure(n * 4)); TRY(s.cost.ensure(n * 8)); TRY(s.pd.ensure(n * H * 8)); TRY(s.crash.ensure(n * 4));
    TRY(s.states(N, Kmax, ego, 5, k, ox, ov));
    TRY(stmpc_solve_batch_device(c, p, N, Kmax, s.ego.as<double>(), s.k.as<int32_t>(), s.ox.as<double>(), s.ov.as<double>(), s.path.as<int32_t>(),
                                 s.bt.as<int32_t>(), s.cost.as<double>(), s.pd.as<double>(), s.crash.as<int32_t>(), nullptr));
    HIPCHK(hipDeviceSynchronize());
    TRY(download(path, s.path, n * H)); TRY(download(bt, s.bt, n)); TRY(download(cost, s.cost, n));
    TRY(download(pd, s.pd, n * H)); TRY(download(crash, s.crash, n));
    stmpc_stats st;
    return stmpc_get_stats(c, &st);
}

int stmpc_solve_grid(stmpc_ctx *c, const uint8_t *obstacles, const double *s_values, int S, const double *t_values,
                     int H, double v0, double a0, const double *distances, double d_w, double v_w, double a_w,
                     double j_w, double v_des, double v_max, double a_min, double a_max, double j_min, double j_max,
                     double min_allowed, double *s_sequence_out) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (!obstacles || !s_values || !t_values || !distances || !s_sequence_out) return fail(STMPC_EINVAL, "NULL host pointer");
    if (bad_layers(H)) return fail(STMPC_EINVAL, "num_t must be in [2, 64]");
    if (S < 2 || S > STMPC_S_LIMIT) return fail(STMPC_EINVAL, "num_s must be in [2, 65000]");
    HIPCHK(hipSetDevice(c->device));
    DevP dp;
    memset(&dp, 0, sizeof dp);
    dp.dt = t_values[1] - t_values[0];           // st_cy.pyx:319
    if (dp.dt == 0.0) return fail(STMPC_EINVAL, "float division by zero (delta_t == 0)");   // ZeroDivisionError in the reference
    if (s_values[1] - s_values[0] == 0.0) return fail(STMPC_EINVAL, "float division by zero (delta_s == 0)");
    dp.dt2 = dp.dt * dp.dt; dp.dt3 = host_pow(dp.dt, 3.0);
    dp.d_w = d_w; dp.v_w = v_w; dp.a_w = a_w; dp.j_w = j_w; dp.v_des = v_des; dp.v_max = v_max; dp.a_min = a_min;
    dp.a_max = a_max; dp.j_min = j_min; dp.j_max = j_max; dp.min_allowed = min_allowed;
    dp.crash_dist_thr = -1.0; dp.H = H;
    auto &s = c->s;
    const size_t cells = (size_t)H * S;
    TRY(s.misc3.ensure((size_t)H * 8));
    TRY(c->solver.counters.ensure(64 * sizeof(unsigned)));
    const int Wg = plan::next_pow2(S + 2 + 128);
    TRY(c->solver.gscratch.ensure((size_t)Wg * STMPC_CELL_BYTES + STMPC_LIST_SLACK + (size_t)Wg * 8));
    TRY(c->solver.bp_tier[STMPC_MAX_TIERS - 1].ensure((size_t)H * Wg * sizeof(u16)));
    TRY(upload(s.misc0, obstacles, cells)); TRY(upload(s.misc1, distances, cells)); TRY(upload(s.misc2, s_values, (size_t)S));
    TRY(latch_solver_error(c));          // an earlier asynchronous call's flag survives the reset below
    HIPCHK(hipMemset(c->solver.counters.p, 0, 64 * sizeof(unsigned)));
    SolveArgs a;
    memset(&a, 0, sizeof a);
    a.p = dp; a.N = 1; a.Kmax = 1; a.W = Wg; a.PW = Wg; a.last_tier = 1;
    for (int i = 0; i < 3; ++i) a.retry_mult[i] = c->solver.knobs.retry_mult[i];
    a.bound_infl = c->solver.knobs.bound_infl; a.last_infl = c->solver.knobs.last_infl;
    a.obstacles = s.misc0.as<uint8_t>(); a.distances = s.misc1.as<double>(); a.s_values = s.misc2.as<double>();
    a.S_grid = S; a.v0_grid = v0; a.a0_grid = a0; a.gsh_max = c->solver.knobs.gsh_max;
    a.bp = c->solver.bp_tier[STMPC_MAX_TIERS - 1].as<u16>(); a.gscratch = c->solver.gscratch.as<unsigned char>(); a.counters = c->solver.counters.as<unsigned>();
    a.s_sequence = s.misc3.as<double>();
    hipLaunchKernelGGL((k_solve<false, true, false, 0, 16, true>), dim3(1), dim3(256), ((stmpc_chunk_ints(Wg) * sizeof(int) + 15) & ~(size_t)15) + 16, nullptr, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    TRY(download(s_sequence_out, s.misc3, (size_t)H));
    unsigned cnt[64];
    HIPCHK(hipMemcpy(cnt, c->solver.counters.p, sizeof cnt, hipMemcpyDeviceToHost));
    if (cnt[STMPC_CNT_ERR]) {
        HIPCHK(hipMemset((unsigned *)c->solver.counters.p + STMPC_CNT_ERR, 0, sizeof(unsigned)));
        return fail(STMPC_EINTERNAL, "grid solver reported a window overflow");
    }
    return STMPC_OK;
}

int stmpc_build_grid(stmpc_ctx *c, const stmpc_params *p, const double *state5, int k, const double *ox,
                     const double *ov, uint8_t *obstacles, double *distances, double *s_values, double *t_values) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (!state5 || !obstacles || !distances || !s_values || !t_values) return fail(STMPC_EINVAL, "NULL host pointer");
    if (k < 0 || k > STMPC_KMAX_LIMIT || (k > 0 && (!ox || !ov))) return fail(STMPC_EINVAL, "bad vehicle count / arrays");
    HIPCHK(hipSetDevice(c->device));
    DevP dp;
    TRY(make_devp(p, &dp));
    const int H = dp.H;
    const double start_s = state5[4];
    const int S = stmpc_num_s(p, start_s);
    if (S < 2 || S > STMPC_S_LIMIT) return fail(STMPC_EINVAL, "number of position cells out of range");
    const int Kalloc = k > 0 ? k : 1;
    auto &s = c->s;
    TRY(c->solver.tab_edge.ensure((size_t)H * Kalloc * 2 * 8));
    TRY(c->solver.tab_win.ensure((size_t)H * Kalloc * 2 * 4));
    TRY(c->solver.tab_nact.ensure((size_t)H * 4));
    TRY(c->solver.tab_nums.ensure(4));
    TRY(c->solver.counters.ensure(64 * sizeof(unsigned)));
    const size_t cells = (size_t)H * S;
    TRY(s.misc0.ensure(cells)); TRY(s.misc1.ensure(cells * 8)); TRY(s.misc2.ensure((size_t)S * 8));
    const int32_t kk = k;
    TRY(s.states(1, k, state5, 5, &kk, ox, ov));
    CarTab tab{c->solver.tab_edge.as<double>(), c->solver.tab_win.as<int>(), c->solver.tab_nact.as<int>(), c->solver.tab_nums.as<int>()};
    unsigned *counters = c->solver.counters.as<unsigned>();
    with_kmax(Kalloc, [&](auto km) {
        launch_predict<decltype(km)::value>(dp, 1, Kalloc, s.ego.as<double>(), s.k.as<int>(), s.ox.as<double>(), s.ov.as<double>(), tab, counters, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, c->sticky.as<unsigned>());
    });
    dim3 grid((S + 255) / 256, H);
    hipLaunchKernelGGL(k_build_grid, grid, dim3(256), 0, nullptr, dp, tab, Kalloc, start_s, S, s.misc0.as<uint8_t>(), s.misc1.as<double>(), s.misc2.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    TRY(download(obstacles, s.misc0, cells)); TRY(download(distances, s.misc1, cells)); TRY(download(s_values, s.misc2, (size_t)S));
    host_t_values(p, H, t_values);
    return STMPC_OK;
}

int stmpc_predict_batch(stmpc_ctx *c, const stmpc_params *p, int mode, int N, int Kmax, const double *ego4,
                        const int32_t *k, const double *ox, const double *ov, const double *sel, double dt,
                        double mcd, double *ego4_out, double *ox_out, double *ov_out, int32_t *crashed) {
    return stmpc_predict_batch_acc(c, p, mode, N, Kmax, ego4, k, ox, ov, sel, dt, mcd, ego4_out, ox_out, ov_out, crashed, nullptr);
}

int stmpc_predict_batch_acc(stmpc_ctx *c, const stmpc_params *p, int mode, int N, int Kmax, const double *ego4,
                            const int32_t *k, const double *ox, const double *ov, const double *sel, double dt,
                            double mcd, double *ego4_out, double *ox_out, double *ov_out, int32_t *crashed, double *oa_out) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    if (N < 0 || Kmax < 0 || Kmax > STMPC_KMAX_LIMIT || (mode != 0 && mode != 1)) return fail(STMPC_EINVAL, "bad N/Kmax/mode");
    if (N == 0) return STMPC_OK;
    if (!ego4 || !k || !ego4_out || !crashed || (mode == 0 && !sel)) return fail(STMPC_EINVAL, "NULL host pointer");
    if (Kmax > 0 && (!ox || !ov || !ox_out || !ov_out)) return fail(STMPC_EINVAL, "NULL host pointer (vehicles)");
    TRY(check_counts(N, Kmax, k));
    HIPCHK(hipSetDevice(c->device));
    DevP dp;
    TRY(make_devp(p, &dp));
    const int Kalloc = Kmax > 0 ? Kmax : 1;
    auto &s = c->s;
    const size_t n = (size_t)N;
    TRY(s.misc0.ensure(n * 8)); TRY(s.misc1.ensure(n * 4 * 8)); TRY(s.misc2.ensure(n * Kalloc * 8)); TRY(s.misc3.ensure(n * Kalloc * 8)); TRY(s.crash.ensure(n * 4));
    if (oa_out) { TRY(s.pd.ensure(n * Kalloc * 8)); HIPCHK(hipMemset(s.pd.p, 0, n * Kalloc * 8)); }
    TRY(s.states(N, Kmax, ego4, 4, k, ox, ov));
    if (mode == 0) TRY(upload(s.misc0, sel, n));
    with_kmax(Kalloc, [&](auto km) {
        hipLaunchKernelGGL(k_predict_step<decltype(km)::value>, dim3((N + 63) / 64), dim3(64), 0, nullptr, dp, mode, N, Kalloc, s.ego.as<double>(), s.k.as<int>(),
                           s.ox.as<double>(), s.ov.as<double>(), s.misc0.as<double>(), dt, mcd, s.misc1.as<double>(), s.misc2.as<double>(), s.misc3.as<double>(),
                           s.crash.as<int>(), oa_out ? s.pd.as<double>() : (double *)nullptr);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    TRY(download(ego4_out, s.misc1, n * 4));
    if (Kmax > 0) { TRY(download(ox_out, s.misc2, n * Kmax)); TRY(download(ov_out, s.misc3, n * Kmax)); }
    TRY(download(crashed, s.crash, n));
    if (Kmax > 0) TRY(download(oa_out, s.pd, n * Kmax));
    return STMPC_OK;
}

int stmpc_fastdiv2_check(double d, double *zl) {
    double z = 0.0;
    const bool ok = fastdiv2_ok(d, &z);
    if (zl) *zl = z;
    return ok ? 1 : 0;
}

int stmpc_probe_arith(stmpc_ctx *c, int op, const double *a, const double *b, double *out, int n) {
    if (!c || !a || !out || n < 0) return fail(STMPC_EINVAL, "bad argument");
    if (n == 0) return STMPC_OK;
    HIPCHK(hipSetDevice(c->device));
    auto &s = c->s;
    TRY(s.misc1.ensure((size_t)n * 8)); TRY(s.misc2.ensure((size_t)n * 8));
    TRY(upload(s.misc0, a, (size_t)n));
    if (b) TRY(upload(s.misc1, b, (size_t)n));
    hipLaunchKernelGGL(k_probe, dim3((n + 255) / 256), dim3(256), 0, nullptr, op, s.misc0.as<double>(), b ? s.misc1.as<double>() : nullptr, s.misc2.as<double>(), n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return download(out, s.misc2, (size_t)n);
}

}  // extern "C"

// ---- solver groups (main.py:43-59, do_grid_search_st): G parameter sets in the launches of one batch ----

int solver_groups_of(const stmpc_params *groups, int G, int n_per_group, int N, SolverGroupsHost *sg) {
    TRY(check_solver_groups(groups, G, n_per_group, &sg->table));
    if ((int64_t)N != (int64_t)G * n_per_group) return fail(STMPC_EINVAL, "N must be G * n_per_group");
    sg->n_per_group = n_per_group;
    return STMPC_OK;
}

extern "C" {

int stmpc_solve_batch_groups_device(stmpc_ctx *c, const stmpc_params *groups, int G, int n_per_group, int N, int Kmax, const double *d_ego, const int32_t *d_k,
                                    const double *d_ox, const double *d_ov, int32_t *d_path, int32_t *d_bt, double *d_cost, double *d_pd, int32_t *d_crash,
                                    double *d_action_cost, void *stream) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    SolverGroupsHost sg;
    TRY(solver_groups_of(groups, G, n_per_group, N, &sg));
    return solve_device(c, &groups[0], &sg, N, Kmax, d_ego, d_k, d_ox, d_ov, d_path, d_bt, d_cost, d_pd, d_crash, d_action_cost, stream);
}

int stmpc_solve_batch_groups(stmpc_ctx *c, const stmpc_params *groups, int G, int n_per_group, int N, int Kmax, const double *ego, const int32_t *k,
                             const double *ox, const double *ov, int32_t *path, int32_t *bt, double *cost, double *pd, int32_t *crash, double *action_cost) {
    if (!c) return fail(STMPC_EINVAL, "ctx is NULL");
    SolverGroupsHost sg;
    TRY(solver_groups_of(groups, G, n_per_group, N, &sg));
    TRY(host_batch_begin(c, N, Kmax, ego, k, ox, ov, path && bt && cost));       // (N = G * n_per_group >= 1)
    const int H = sg.table[0].p.H;
    auto &s = c->s;
    const size_t n = (size_t)N;
    TRY(s.path.ensure(n * H * 4)); TRY(s.bt.ensure(n * 4)); TRY(s.cost.ensure(n * 8)); TRY(s.pd.ensure(n * H * 8)); TRY(s.crash.ensure(n * 4));
    TRY(s.f_out.ensure(n * 2 * 8));               // (the action_cost rows)
    TRY(s.states(N, Kmax, ego, 5, k, ox, ov));
    TRY(solve_device(c, &groups[0], &sg, N, Kmax, s.ego.as<double>(), s.k.as<int32_t>(), s.ox.as<double>(), s.ov.as<double>(), s.path.as<int32_t>(),
                     s.bt.as<int32_t>(), s.cost.as<double>(), s.pd.as<double>(), s.crash.as<int32_t>(), action_cost ? s.f_out.as<double>() : nullptr, nullptr));
    HIPCHK(hipDeviceSynchronize());
    TRY(download(path, s.path, n * H)); TRY(download(bt, s.bt, n)); TRY(download(cost, s.cost, n));
    TRY(download(pd, s.pd, n * H)); TRY(download(crash, s.crash, n)); TRY(download(action_cost, s.f_out, n * 2));
    stmpc_stats st;
    return stmpc_get_stats(c, &st);
}

}  // extern "C"
