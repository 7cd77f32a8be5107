// Prints the route a far-field transform call takes (metalens_amd/csrc/transform_route.h) for plan facts given as
// name=value arguments; what is not given keeps the default below, and beside it the kernel each GEMM-path stage
// launches for those facts: zfold/<wide|narrow>/<f64|f32>/<plain|in_sum|out_t> or zgemm/<tile id>, with the split-K
// slabs it writes (f32=1: the fp32 mode of the folded GEMMs); for an FFT stage the kernel zfft.hip launches
// (transform_route.h zfft_launch_rule) as zfft/one/R<R3T>/p<PASS>[/ip], zfft/pass/R<R3P>x<P>/p<PASS>, zfft/multi/p<PASS>,
// zfft/tiles, zfft/interleaved, zfft/cols128 (zfft/none: no kernel takes the facts) and the launches it takes.
// y.lattice=N (x.lattice=N): the axis as plan_fft_axis plans a grid of my (mx) bins on the lattice of N samples, every
// y.jstep-th a wanted one, under `method` (zfft_axis_rule) - instead of y.ok, y.N, y.split, y.passes given one by one;
// y.M / x.M: the wanted bins where they are not my / mx.  n_ranks=G with shard=2: the interleaved shard's block as
// interleave_block_of gives it, unless block= is given.  `lattice n step wavelength n_glass u...`: which lattice
// plan_fft_axis finds for an axis and its direction grid.  `fold n step wavelength n_glass u...`: whether that axis takes
// the folded GEMM, over how many half-directions, and the split directions the planner uploads (fold_split), the
// doubles as %a.  Runs without a GPU.
// Build + run:  make -C tools transform_route && tools/transform_route ny=4096 nx_total=4096 nxl=4096 mx=512 my=512 \
//                   y.ok=1 y.N=4096 x.ok=1 x.N=4096 row_first=1 trim_lo=150 trim_hi=3946
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "transform_route.h"

using namespace ml;

// `lattice n step wavelength n_glass u[0] u[1] ...` (floating-point values as strtod reads them, hex included): the
// lattice plan_fft_axis finds for that axis (transform_route.h zfft_axis_lattice)
static int lattice_main(int argc, char **argv) {
    if (argc < 8) return fprintf(stderr, "usage: %s lattice n step wavelength n_glass u[0] u[1] ...\n", argv[0]), 2;
    std::vector<double> u;
    for (int i = 6; i < argc; ++i) u.push_back(strtod(argv[i], nullptr));
    int N_eff = 0, j0 = 0, jstep = 1, N_plain = 0;
    const bool ok = zfft_axis_lattice(atoi(argv[2]), strtod(argv[3], nullptr), strtod(argv[4], nullptr),
                                      strtod(argv[5], nullptr), u.data(), (int)u.size(), &N_eff, &j0, &jstep, &N_plain);
    printf("ok=%d N_eff=%d j0=%d jstep=%d N_plain=%d\n", ok, N_eff, j0, jstep, N_plain);
    return 0;
}

// `fold n step wavelength n_glass u[0] u[1] ...`: what the planner of a folded GEMM axis finds for that axis
// (transform_route.h fold_split); v = hi[S], lo[S], then u_c as (hi, lo)
static int fold_main(int argc, char **argv) {
    if (argc < 7) return fprintf(stderr, "usage: %s fold n step wavelength n_glass u[0] u[1] ...\n", argv[0]), 2;
    std::vector<double> u;
    for (int i = 6; i < argc; ++i) u.push_back(strtod(argv[i], nullptr));
    const FoldSplit f = fold_split(u.data(), (int)u.size(), atoi(argv[2]), strtod(argv[3], nullptr),
                                   strtod(argv[4], nullptr), strtod(argv[5], nullptr));
    printf("ok=%d S=%d has_E=%d v=", f.ok, f.S, f.has_E);
    for (size_t k = 0; k < f.v.size(); ++k) printf("%s%a", k ? "," : "", f.v[k]);
    printf("\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "lattice")) return lattice_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "fold")) return fold_main(argc, argv);
    std::map<std::string, long> a = {{"method", ML_METHOD_AUTO}, {"nx_total", 0}, {"ny", 0}, {"mx", 0}, {"my", 0},
        {"pair_list", 0}, {"fold", 0}, {"fold_S", 0}, {"fold2", 0}, {"fold2_S", 0}, {"nxl", 0}, {"shard", 0}, {"row0", 0},
        {"row_first", 0}, {"trim_lo", 0}, {"trim_hi", 0}, {"f32", 0}, {"y.ok", 0}, {"y.N", 0}, {"y.split", 1}, {"y.passes", 0},
        {"y.A", 0}, {"x.ok", 0}, {"x.N", 0}, {"x.split", 1}, {"x.passes", 0}, {"x.A", 0},
        {"y.lattice", 0}, {"y.jstep", 1}, {"y.M", -1}, {"x.lattice", 0}, {"x.jstep", 1}, {"x.M", -1},
        {"n_ranks", 1}, {"block", -1},
        // the diagnostic knobs (RouteKnobs), by their environment names; -1: the default
        {"ML_STAGE1_SPLIT", -1}, {"ML_G_SKEW", -1}, {"ML_G_TILED", -1}, {"ML_FOLD2_MIN_TILES", -1},
        {"ML_NO_ROW_TRIM", -1}, {"ML_NO_GT_DIRECT", -1}};
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        const std::string name(argv[i], eq ? eq - argv[i] : 0);
        if (!a.count(name)) return fprintf(stderr, "unknown argument %s\n", argv[i]), 2;
        a[name] = atol(eq + 1);
    }
    PlanFacts pl;
    pl.method = a["method"], pl.nx_total = a["nx_total"], pl.ny = a["ny"], pl.mx = a["mx"], pl.my = a["my"];
    pl.pair_list = a["pair_list"], pl.fold = a["fold"], pl.fold_S = a["fold_S"], pl.fold2 = a["fold2"];
    pl.fold2_S = a["fold2_S"];
    ZfftAxisGeo ax[2];
    for (int k = 0; k < 2; ++k) {
        const std::string p = k ? "x." : "y.";
        ax[k].ok = a[p + "ok"], ax[k].N_eff = a[p + "N"], ax[k].split = a[p + "split"];
        ax[k].passes = a[p + "passes"], ax[k].A = a[p + "A"], ax[k].jstep = a[p + "jstep"];
        if (a[p + "M"] < 0) a[p + "M"] = k ? pl.mx : pl.my;
        if (a[p + "lattice"] > 0) {
            const ZfftAxisRule rule = zfft_axis_rule(pl.method, a[p + "lattice"], ax[k].jstep, a[p + "M"]);
            ax[k].ok = rule.taken && rule.split > 0;
            ax[k].N_eff = a[p + "lattice"], ax[k].split = rule.split, ax[k].passes = rule.passes;
        }
    }
    Shard sh;
    sh.kind = (ShardKind)a["shard"];   // 0 block, 1 mirrored, 2 interleaved
    sh.row0 = a["row0"];
    sh.n_ranks = a["n_ranks"];
    sh.block = a["block"] >= 0 ? (int)a["block"]
               : ax[1].ok && !ax[1].A ? interleave_block_of(ax[1].N_eff, pl.nx_total, sh.n_ranks) : 0;
    const int trim[2] = {(int)a["trim_lo"], (int)a["trim_hi"]};
    RouteKnobs kn;
    auto knob = [&a](const char *name, auto &value) { if (a[name] >= 0) value = a[name]; };
    knob("ML_STAGE1_SPLIT", kn.stage1_split), knob("ML_G_SKEW", kn.g_skew), knob("ML_G_TILED", kn.g_tiled);
    knob("ML_FOLD2_MIN_TILES", kn.fold2_min_tiles), knob("ML_NO_ROW_TRIM", kn.no_row_trim);
    knob("ML_NO_GT_DIRECT", kn.no_gt_direct);
    const TransformRoute rt = transform_route(pl, ax[0], ax[1], sh, a["nxl"], a["row_first"] != 0, trim, kn);
    static const char *const s1[] = {"fft", "folded", "generic"}, *const lay[] = {"row_major", "transposed", "tiled"};
    static const char *const s2[] = {"interleaved", "fft", "fft_tiles", "folded", "generic_mirrored", "generic", "coldot"};
    printf("stage1=%s want_split1=%d g_transposed=%d g_layout=%s g_ld=%lld g_bytes=%zu pieces_wanted=%d trim_lo=%d "
           "trim_hi=%d gt_direct=%d stage2=%s", s1[(int)rt.stage1], rt.want_split1, rt.g_transposed(),
           lay[(int)rt.g_layout], (long long)rt.g_ld, rt.g_bytes, rt.pieces_wanted, rt.trim_lo, rt.trim_hi, rt.gt_direct,
           s2[(int)rt.stage2]);
    // the kernels behind the stage kinds, as the launchers pick them (farfield.hip stage1, stage2_folded,
    // stage2_generic; zfold.hip zfold_stage1; zgemm.hip zgemm)
    const int nxl = a["nxl"];
    const char *const prec = a["f32"] ? "f32" : "f64";
    auto zfold_name = [prec](int M, int S, int splits, const char *io) {
        return std::string("zfold/") + (zfold_take_wide(M, S, splits) ? "wide/" : "narrow/") + prec + "/" + io;
    };
    std::string k1 = s1[(int)rt.stage1], k2 = s2[(int)rt.stage2];
    int splits1 = 1, splits2 = 1, launches2 = 1;
    if (rt.stage1 == Stage1Kind::folded) {
        splits1 = zfold_eff_splits((pl.ny + 1) / 2, rt.want_split1);
        k1 = zfold_name(4 * nxl, pl.fold_S, splits1, rt.gt_direct ? "out_t" : "plain");
    } else if (rt.stage1 == Stage1Kind::generic) {
        k1 = "zgemm/" + std::to_string(zgemm_tile(4 * nxl, pl.my, 1));
    }
    if (rt.stage2 == Stage2Kind::folded) {
        // (stage 1's slabs are summed on the way in where it wrote them transposed; else the transposer sums them)
        splits2 = zfold_eff_splits((nxl + 1) / 2, fold2_want_split(pl.my, pl.fold2_S));
        k2 = zfold_name(4 * pl.my, pl.fold2_S, splits2, rt.gt_direct && splits1 > 1 ? "in_sum" : "plain");
    } else if (rt.stage2 == Stage2Kind::generic || rt.stage2 == Stage2Kind::generic_mirrored) {
        launches2 = rt.stage2 == Stage2Kind::generic_mirrored ? 2 : 1;   // one GEMM per run of resident rows
        k2 = "zgemm/" + std::to_string(zgemm_tile(pl.mx, pl.my, 4));
    }
    // the FFT stages, as farfield.hip stage1_fft, stage2_fft and stage2_interleaved fill their calls
    auto zfft_name = [](const ZfftLaunchFacts &f) {
        const ZfftLaunch L = zfft_launch_rule(f);
        const std::string pass = "/p" + std::to_string(L.PASS);
        switch (L.family) {
            case ZfftFamily::one: return "zfft/one/R" + std::to_string(L.R3T) + pass + (L.ip ? "/ip" : "");
            case ZfftFamily::pass: return "zfft/pass/R" + std::to_string(L.R3P) + "x" + std::to_string(L.P) + pass;
            case ZfftFamily::multi: return "zfft/multi" + pass;
            case ZfftFamily::tiles: return std::string("zfft/tiles");
            case ZfftFamily::interleaved: return std::string("zfft/interleaved");
            case ZfftFamily::cols128: return std::string("zfft/cols128");
            default: return std::string("zfft/none");
        }
    };
    int launches1 = 1, threads1 = 0, threads2 = 0, stuff = 0;
    const GView gv = g_view(rt.g_layout, nxl, pl.my, rt.g_ld, rt.trim_lo);
    if (rt.stage1 == Stage1Kind::fft) {
        ZfftLaunchFacts f;
        f.N_eff = ax[0].N_eff / std::max(ax[0].split, 1), f.M = a["y.M"], f.passes = ax[0].passes;
        f.contiguous = true, f.tiled_out = rt.g_layout == GLayout::tiled;
        k1 = ax[0].A ? std::string("zfft_mixed") : zfft_name(f);
        threads1 = zfft_launch_rule(f).threads;
        launches1 = ax[0].split;
    }
    if (rt.stage2 == Stage2Kind::interleaved && sh.block > 0) {
        ZfftLaunchFacts f;
        const int sG = sh.block * sh.n_ranks;
        stuff = interleave_stuff(ax[1].N_eff / sG);
        f.N_eff = ax[1].N_eff / sG * stuff, f.M = a["x.M"], f.s = sh.block, f.stuff = stuff, f.n_valid = pl.nx_total / sG;
        k2 = zfft_name(f);
        threads2 = zfft_launch_rule(f).threads;
    } else if (rt.stage2 == Stage2Kind::fft || rt.stage2 == Stage2Kind::fft_tiles) {
        ZfftLaunchFacts f;
        f.N_eff = ax[1].N_eff / std::max(ax[1].split, 1), f.M = a["x.M"], f.passes = ax[1].passes;
        f.contiguous = gv.s_row == 1, f.second = rt.g_layout == GLayout::transposed;
        f.tiles = rt.stage2 == Stage2Kind::fft_tiles;
        k2 = ax[1].A ? std::string("zfft_mixed") : zfft_name(f);
        threads2 = zfft_launch_rule(f).threads;
        launches2 = f.tiles ? 1 : ax[1].split;
    }
    printf(" stage1_kernel=%s stage1_splits=%d stage1_launches=%d stage2_kernel=%s stage2_splits=%d stage2_launches=%d",
           k1.c_str(), splits1, launches1, k2.c_str(), splits2, launches2);
    printf(" stage1_threads=%d stage2_threads=%d y.ok=%d y.split=%d y.passes=%d x.ok=%d x.split=%d x.passes=%d block=%d "
           "stuff=%d\n", threads1, threads2, ax[0].ok, ax[0].split, ax[0].passes, ax[1].ok, ax[1].split, ax[1].passes,
           sh.block, stuff);
    return 0;
}
