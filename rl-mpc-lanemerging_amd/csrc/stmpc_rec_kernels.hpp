// stmpc_rec_kernels.hpp -- the episode flight recorder next to the batched world of stmpc_cc_kernels.hpp (sim::): what the reference's
// control.run_episode keeps per tick (state_history, position / speed / acceleration / jerk histories, control.py:280-289; the combined
// controller's takeover_history, dqn.py:101-115) and what stats.StatsAggregator and RLAgent.plot_st_proportion bin over the ego's x
// (stats.py:33-52, dqn.py:215-226), for N environments, without anything crossing to the host.
//   k_rec_tick    called between the controller and sim::k_sim_step with the view arrays the controller consumed.  For every environment whose
//                 status is still 0: one record into slot (world tick mod T) of that environment's ring, and the tick added to the environment's
//                 bin accumulators.  A workgroup of 256 threads serves REC_G environments: its four waves copy the records with the lanes
//                 laid across the COLUMNS of a record (the [N][Kmax] view rows are read and the ring rows written as contiguous runs), and
//                 its first REC_G threads do the per-environment arithmetic (jerk, bins) on arrays whose fastest index is the environment.
//                 No cross-environment reduction, no atomics.
//   k_rec_reduce  one workgroup per accumulator row (bin x quantity, then the two per-environment totals): every thread adds its environments
//                 in index order, the 256 partial sums are added by a fixed tree through LDS.  The order depends on N alone.
// Record (REC_HDR + 3 Kmax doubles): world tick, ego x, y, v, a, s, k, commanded speed, takeover flag, jerk, then x / v / a of the Kmax view slots.
// The jerk is the reference's jerk_history entry: 0 for the first record of an episode, else (a_t - a_{t-1}) / TICK_LENGTH with the recorder's
// own previous acceleration (control.py:285-289).
#pragma once
#include "stmpc_cc_kernels.hpp"

namespace stmpc {
namespace rec {

constexpr int HDR = 10;                     // STMPC_REC_HDR
enum { C_TICK = 0, C_X = 1, C_Y = 2, C_V = 3, C_A = 4, C_S = 5, C_K = 6, C_CMD = 7, C_TAKEOVER = 8, C_JERK = 9 };
constexpr int MAX_EDGES = 32;               // STMPC_REC_MAX_EDGES
constexpr int NQ = 4;                       // STMPC_REC_NQ: count, takeover count, sum |jerk|, sum |speed| per bin
enum { Q_COUNT = 0, Q_TAKEOVER = 1, Q_JERK = 2, Q_SPEED = 3 };
constexpr int G = 8;                        // environments per workgroup of k_rec_tick
constexpr int THREADS = 256;

struct Cfg {
    int N, Kmax, T, n_edges;
    double tick;                            // Settings.TICK_LENGTH
    double edges[MAX_EDGES];
};
struct State {                              // device arrays
    double *ring;                           // [N][T][HDR + 3 Kmax]
    int *nrec;                              // [N] records written since the reset
    int *last_tick;                         // [N] world tick of the newest record
    double *prev_a;                         // [N] the ego's acceleration in the newest record
    double *acc;                            // [NQ * (n_edges - 1) + 2][N]: per quantity and bin, then takeovers and controlled ticks; environment fastest
    double *red;                            // [NQ * (n_edges - 1) + 2] the rows of acc summed over the environments (k_rec_reduce)
};
__host__ __device__ inline int row_width(int Kmax) { return HDR + 3 * Kmax; }
__host__ __device__ inline int acc_rows(int n_edges) { return NQ * (n_edges - 1) + 2; }

// np.histogram's rule (stats.py:45, dqn.py:217-218): edge[b] <= x < edge[b + 1], the last bin closed on the right; -1 = outside
__device__ __forceinline__ int bin_hist(const Cfg &c, double x) {
    const int nb = c.n_edges - 1;
    if (!(x >= c.edges[0]) || !(x <= c.edges[nb])) return -1;
    int b = 0;
    while (b + 1 < nb && x >= c.edges[b + 1]) ++b;
    return b;
}
// the loop of stats.py:48-52: the first b with x <= edge[b + 1] (the ego's x never decreases, so the reference's running index is this one);
// x below the first edge lands in bin 0; -1 beyond the last edge, where the reference's loop runs off its array
__device__ __forceinline__ int bin_loop(const Cfg &c, double x) {
    const int nb = c.n_edges - 1;
    int b = 0;
    while (b < nb && x > c.edges[b + 1]) ++b;
    return b < nb ? b : -1;
}

__global__ void __launch_bounds__(THREADS) k_rec_tick(Cfg c, State r, const int *__restrict__ status, const int *__restrict__ ticks,
                                                      const double *__restrict__ ego5, const int *__restrict__ k_count, const double *__restrict__ ox,
                                                      const double *__restrict__ ov, const double *__restrict__ oa, const double *__restrict__ cmd,
                                                      const int *__restrict__ takeover) {
    const int e0 = blockIdx.x * G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = row_width(c.Kmax), K = c.Kmax;
    // the records: a wave per environment, lanes across the columns (the jerk column belongs to the environment's thread below)
    for (int g = wave; g < G; g += THREADS / 64) {
        const int e = e0 + g;
        if (e >= c.N || status[e] != 0) continue;
        const int tk = ticks[e];
        double *row = r.ring + ((size_t)e * c.T + (size_t)(tk % c.T)) * W;
        for (int col = lane; col < W; col += 64) {
            double v;
            if (col >= HDR) {
                const int q = col - HDR;
                const size_t at = (size_t)e * K + (q < K ? q : (q < 2 * K ? q - K : q - 2 * K));
                v = q < K ? ox[at] : (q < 2 * K ? ov[at] : (oa ? oa[at] : 0.0));
            } else if (col == C_TICK) v = (double)tk;
            else if (col <= C_S) v = ego5[(size_t)e * 5 + (col - C_X)];
            else if (col == C_K) v = (double)k_count[e];
            else if (col == C_CMD) v = cmd[e];
            else if (col == C_TAKEOVER) v = takeover ? (double)(takeover[e] != 0) : 0.0;
            else continue;
            row[col] = v;
        }
    }
    // per environment: the jerk column, the recorder's own bookkeeping and the bin accumulators
    if (threadIdx.x < G) {
        const int e = e0 + threadIdx.x;
        if (e >= c.N || status[e] != 0) return;
        const int tk = ticks[e], n = r.nrec[e];
        const double x = ego5[(size_t)e * 5 + 0], v = ego5[(size_t)e * 5 + 2], a = ego5[(size_t)e * 5 + 3];
        const double jerk = n == 0 ? 0.0 : (a - r.prev_a[e]) / c.tick;
        r.ring[((size_t)e * c.T + (size_t)(tk % c.T)) * W + C_JERK] = jerk;
        r.prev_a[e] = a; r.nrec[e] = n + 1; r.last_tick[e] = tk;
        const int nb = c.n_edges - 1;
        const size_t N = (size_t)c.N;
        const bool took = takeover && takeover[e] != 0;
        const int bh = bin_hist(c, x), bl = bin_loop(c, x);
        if (bh >= 0) {
            r.acc[((size_t)Q_COUNT * nb + bh) * N + e] += 1.0;
            if (took) r.acc[((size_t)Q_TAKEOVER * nb + bh) * N + e] += 1.0;
        }
        if (bl >= 0) {
            r.acc[((size_t)Q_JERK * nb + bl) * N + e] += fabs(jerk);
            r.acc[((size_t)Q_SPEED * nb + bl) * N + e] += fabs(v);
        }
        if (took) r.acc[((size_t)NQ * nb + 0) * N + e] += 1.0;
        r.acc[((size_t)NQ * nb + 1) * N + e] += 1.0;
    }
}

__global__ void __launch_bounds__(THREADS) k_rec_reduce(int N, const double *__restrict__ acc, double *__restrict__ red) {
    __shared__ double part[THREADS];
    const double *row = acc + (size_t)blockIdx.x * N;
    double s = 0.0;
    for (int e = threadIdx.x; e < N; e += THREADS) s += row[e];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) red[blockIdx.x] = part[0];
}

}  // namespace rec
}  // namespace stmpc
