// Prints the route a far-field transform call takes (metalens_amd/csrc/transform_route.h) for plan facts given as
// name=value arguments; what is not given keeps the default below, and beside it the kernel each GEMM-path stage
// launches for those facts: zfold/<wide|narrow>/<f64|f32>/<plain|in_sum|out_t> or zgemm/<tile id>, with the split-K
// slabs it writes (f32=1: the fp32 mode of the folded GEMMs).  Runs without a GPU.
// Build + run:  make -C tools transform_route && tools/transform_route ny=4096 nx_total=4096 nxl=4096 mx=512 my=512 \
//                   y.ok=1 y.N=4096 x.ok=1 x.N=4096 row_first=1 trim_lo=150 trim_hi=3946
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "transform_route.h"

using namespace ml;

int main(int argc, char **argv) {
    std::map<std::string, long> a = {{"method", ML_METHOD_AUTO}, {"nx_total", 0}, {"ny", 0}, {"mx", 0}, {"my", 0},
        {"pair_list", 0}, {"fold", 0}, {"fold_S", 0}, {"fold2", 0}, {"fold2_S", 0}, {"nxl", 0}, {"shard", 0}, {"row0", 0},
        {"row_first", 0}, {"trim_lo", 0}, {"trim_hi", 0}, {"f32", 0}, {"y.ok", 0}, {"y.N", 0}, {"y.split", 1}, {"y.passes", 0},
        {"y.A", 0}, {"x.ok", 0}, {"x.N", 0}, {"x.split", 1}, {"x.passes", 0}, {"x.A", 0},
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
        ax[k].passes = a[p + "passes"], ax[k].A = a[p + "A"];
    }
    Shard sh;
    sh.kind = (ShardKind)a["shard"];   // 0 block, 1 mirrored, 2 interleaved
    sh.row0 = a["row0"];
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
    printf(" stage1_kernel=%s stage1_splits=%d stage2_kernel=%s stage2_splits=%d stage2_launches=%d\n", k1.c_str(),
           splits1, k2.c_str(), splits2, launches2);
    return 0;
}
