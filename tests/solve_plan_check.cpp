// Prints the launch plan of one batched solve (csrc/stmpc_solve_plan.hpp) -- host code only, for tests/test_solve_plan_cpu.py.
// usage: solve_plan_check num_cu lds_per_block N Kmax grouped fastdiv_proven H future_s ds dt dt2 dt3 v_w a_w j_w v_des v_max a_min a_max j_min j_max
//        solve_plan_check variants        (every instantiation variant_built lists, one name per line)
//        solve_plan_check reachable num_cu lds_per_block H future_s ... j_max      (every variant some setting of the knobs that choose kernels launches
//                                         on that lattice, built or not, one name per line -- for tests/test_solver_variants_cpu.py)
// The settings come from the STMPC_* environment, as in stmpc_create.  History is a fresh context's; the checkpoint pool is taken as granted
// wherever the plan wants it (a fresh context on a device with memory to spare).
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>

#include "stmpc_solve_plan.hpp"

using namespace stmpc::plan;

// the fields of DevP the plan reads
struct Params { int H; double future_s, ds, dt, dt2, dt3, v_w, a_w, j_w, v_des, v_max, a_min, a_max, j_min, j_max; };

static std::string name_of(const KernelVariant &v) {
    char buf[160];
    snprintf(buf, sizeof buf, "%sk_solve<%s, false, %s, %d, %d, %s, %d, %d>", v.grouped ? "grouped::" : "", v.use_lds ? "true" : "false", v.fastdiv ? "true" : "false",
             v.kt, v.fanmax, v.s1gen ? "true" : "false", v.res, v.nwx);
    return buf;
}

static std::string render(const SolvePlan &p) {
    static const char *streams[] = {"main", "side", "masked", "reserved"}, *events[] = {"-", "fork", "join", "join0", "join_r", "dp_end"}, *ops[] = {"none", "solve", "order", "order8"};
    std::string out;
    char buf[320];
    snprintf(buf, sizeof buf, "plan nt %d S_nom %d Wg %d small_fan %d stage_tab %d fastdiv %d prune %d need_hbm %d bp_elem %zu ckpt_stride %zu pool_cap %d pool_bytes %zu resume_wanted %d "
             "overlap %d split %d heavy_first %d reserve %d two_phase %d guided %d side_grid %d maxshift %d band %.17g band2_mult %.17g\n", p.nt, p.S_nom, p.Wg, p.small_fan, p.stage_tab,
             p.fastdiv, p.prune_on, p.need_hbm_tier, p.bp_elem, p.ckpt_stride, p.pool_cap, p.pool_bytes, p.resume_wanted, p.overlap, p.split, p.heavy_first, p.reserve, p.two_phase,
             p.guided, p.side_grid, p.maxshift, p.band, p.band2_mult);
    out += buf;
    for (int i = 0; i < p.nt; ++i) {
        const PlanTier &t = p.tier[i];
        snprintf(buf, sizeof buf, "tier %d W %d PW %d waves %d grid %d lds_bytes %zu lds %d\n", i, t.W, t.PW, t.waves, t.grid, t.lds_bytes, t.lds);
        out += buf;
    }
    for (int i = 0; i < p.n_steps; ++i) {
        const PlanStep &s = p.steps[i];
        snprintf(buf, sizeof buf, "step %s stream %s wait %s record %s tier %d phase %d\n", ops[(int)s.op], streams[(int)s.stream], events[(int)s.wait], events[(int)s.record], s.tier, s.phase);
        out += buf;
        if (s.op != Op::Solve) continue;
        const PlanTier &t = p.tier[s.tier];
        const KernelVariant &v = p.resume_wanted ? t.variant_resume : t.variant;
        snprintf(buf, sizeof buf, "launch %s | grid %d block %d lds %zu built %d\n", name_of(v).c_str(), s.grid, 64 * t.waves, t.lds_bytes, variant_built(v) ? 1 : 0);
        out += buf;
    }
    return out;
}

// The knobs that decide which kernels a solve launches, swept in-process: windows, waves per workgroup, staged table, division, resume, bounded
// search and penalty-buffer cells, lone and grouped, with and without vehicles and past the staged table's eight, at N below and above one
// workgroup per compute unit.  (The other knobs reach the kernels as arguments, or move grids and streams.)
static std::set<std::string> reachable(const DeviceShape &dev, const Params &dp) {
    static const int tiers[][4] = {{0}, {1, 64}, {2, 256, 512}, {2, 512, 2048}, {3, 64, 128, 256}, {2, 2048, 8192}};
    static const int waves[][3] = {{0, 0, 0}, {4, 0, 0}, {8, 0, 0}, {0, 8, 4}, {0, 4, 8}};      // {STMPC_NW=n, or "a,b"}
    static const int pens[] = {0, 256, 512};
    std::set<std::string> met;
    for (const auto &tw : tiers) for (const auto &nw : waves) for (int pen : pens) for (int bits = 0; bits < 16; ++bits) for (int prune = -1; prune <= 1; ++prune) {
        SolveKnobs k;
        k.max_waves_per_cu = 4;
        if (tw[0] > 0) { k.n_lds_tiers = tw[0]; k.tiers_from_env = true; for (int i = 0; i < tw[0]; ++i) k.lds_tier_W[i] = tw[1 + i]; }
        k.waves_override = nw[0]; k.waves_tier[0] = nw[1]; k.waves_tier[1] = nw[2];
        k.pen_cells[0] = k.pen_cells[1] = pen;
        k.allow_stage_tab = (bits & 1) != 0; k.resume = (bits & 2) != 0; k.prune = prune;
        SolveHistory hist;
        hist.fastdiv_proven = (bits & 4) != 0;
        const bool grouped = (bits & 8) != 0;
        for (int N : {200, 600, 4096}) for (int Kmax : {0, 8, 9}) {
            const SolvePlan p = plan_solve(k, dev, dp, N, Kmax, grouped, hist);
            for (int i = 0; i < p.n_steps; ++i)
                if (p.steps[i].op == Op::Solve) met.insert(name_of(p.resume_wanted ? p.tier[p.steps[i].tier].variant_resume : p.tier[p.steps[i].tier].variant));
        }
    }
    return met;
}

static void read_params(char **argv, Params *dp) {
    dp->H = atoi(argv[0]);
    double *f[] = {&dp->future_s, &dp->ds, &dp->dt, &dp->dt2, &dp->dt3, &dp->v_w, &dp->a_w, &dp->j_w, &dp->v_des, &dp->v_max, &dp->a_min, &dp->a_max, &dp->j_min, &dp->j_max};
    for (int i = 0; i < 14; ++i) *f[i] = strtod(argv[1 + i], nullptr);
}

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "variants") {
        const int fans[] = {9, STMPC_FAN1, STMPC_FAN88}, nwxs[] = {4, STMPC_MAXWAVES, 88};
        for (int bits = 0; bits < 16; ++bits) for (int kt : {0, 8}) for (int fi = 0; fi < 3; ++fi) for (int res = 0; res < 3; ++res) for (int nwx : nwxs) {
            if (fi > 0 && fans[fi] == fans[fi - 1]) continue;
            const KernelVariant v{(bits & 1) != 0, (bits & 2) != 0, kt, fans[fi], (bits & 4) != 0, res, nwx, (bits & 8) != 0};
            if (variant_built(v)) puts(name_of(v).c_str());
        }
        return 0;
    }
    if (argc == 19 && std::string(argv[1]) == "reachable") {
        Params dp;
        read_params(argv + 4, &dp);
        for (const std::string &name : reachable(DeviceShape{atoi(argv[2]), atoi(argv[3])}, dp)) puts(name.c_str());
        return 0;
    }
    if (argc != 22) { fprintf(stderr, "solve_plan_check: 21 arguments expected, %d given\n", argc - 1); return 2; }
    const DeviceShape dev{atoi(argv[1]), atoi(argv[2])};
    const int N = atoi(argv[3]), Kmax = atoi(argv[4]);
    const bool grouped = atoi(argv[5]) != 0;
    SolveHistory hist;
    hist.fastdiv_proven = atoi(argv[6]) != 0;
    Params dp;
    read_params(argv + 7, &dp);
    const SolveKnobs knobs = SolveKnobs::from_env();
    const std::string once = render(plan_solve(knobs, dev, dp, N, Kmax, grouped, hist)), twice = render(plan_solve(knobs, dev, dp, N, Kmax, grouped, hist));
    fputs(once.c_str(), stdout);
    printf("pure %d\n", once == twice ? 1 : 0);
    return 0;
}
