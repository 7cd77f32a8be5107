// The device arithmetic of metalens_amd/csrc/nearfield_math.h on the host, for tests/test_device_math_host.py and
// tests/test_gpu_device_math.py.  Compile without contraction (-ffp-contract=off, as the library is).
//
// sincos_cw, reduce_pio2 and sincos_cw_q are rint / fma / multiply / int-convert only, so they are RESTATED here
// operation by operation - std::fma wherever the header has fma() or horner() - and give the device's bits:
//   device_math sincos   X OUT        X: n doubles;            OUT: sin[n], cos[n]
//   device_math sincos_q X KQ OUT     KQ: n int32 quadrants;   OUT: sin[n], cos[n] of x + kq pi/2
//   device_math reduce   X OUT                                 OUT: r[n] doubles, then k[n] int32
// sqrt_exact, recip and rsqrt_fast start from a hardware estimate the host does not have.  They are MODELLED: the
// estimate is the correctly rounded 1 / sqrt(x) or 1 / x times (1 + u eps), u in [-1, 1] - every fourth value at an end
// of the interval, the others drawn from a generator seeded by SEED - followed by the header's own sequence:
//   device_math model sqrt|recip|rsqrt EPS SEED X OUT          OUT: n doubles
// Files are raw host-endian arrays.  Nothing here runs on a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

// ---- the restatement (nearfield_math.h, line by line) ----

// (the header's horner is one v_fma_f64: p = z * p + C)
double horner(double z, double p, double C) { return std::fma(z, p, C); }

void sincos_cw(double x, double &s, double &c) {
    const double k = std::rint(x * 0.63661977236758138243);          // 2/pi
    double r = std::fma(-k, 1.57079632679489655800e+00, x);          // pi/2 hi
    r = std::fma(-k, 6.12323399573676603587e-17, r);                 // pi/2 mid
    const double z = r * r;
    double ps = horner(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    ps = horner(z, ps, 2.75573137070700676789e-06);
    ps = horner(z, ps, -1.98412698298579493134e-04);
    ps = horner(z, ps, 8.33333333332248946124e-03);
    ps = horner(z, ps, -1.66666666666666324348e-01);
    const double sn = std::fma(z * r, ps, r);
    double pc = horner(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    pc = horner(z, pc, -2.75573143513906633035e-07);
    pc = horner(z, pc, 2.48015872894767294178e-05);
    pc = horner(z, pc, -1.38888888888741095749e-03);
    pc = horner(z, pc, 4.16666666666666019037e-02);
    const double cs = std::fma(z * z, pc, std::fma(z, -0.5, 1.0));
    const int q = (int)k & 3;
    const double a = (q & 1) ? cs : sn, b = (q & 1) ? sn : cs;
    s = (q & 2) ? -a : a;
    c = ((q + 1) & 2) ? -b : b;
}

void reduce_pio2(double x, double &r, int &k) {
    const double kd = std::rint(x * 0.63661977236758138243);
    r = std::fma(-kd, 1.57079632679489655800e+00, x);
    r = std::fma(-kd, 6.12323399573676603587e-17, r);
    k = (int)kd;
}

void sincos_cw_q(double x, int kq, double &s, double &c) {
    const double k = std::rint(x * 0.63661977236758138243);          // 2/pi
    double r = std::fma(-k, 1.57079632679489655800e+00, x);          // pi/2 hi
    r = std::fma(-k, 6.12323399573676603587e-17, r);                 // pi/2 mid
    const double z = r * r;
    double ps = horner(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    ps = horner(z, ps, 2.75573137070700676789e-06);
    ps = horner(z, ps, -1.98412698298579493134e-04);
    ps = horner(z, ps, 8.33333333332248946124e-03);
    ps = horner(z, ps, -1.66666666666666324348e-01);
    const double sn = std::fma(z * r, ps, r);
    double pc = horner(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    pc = horner(z, pc, -2.75573143513906633035e-07);
    pc = horner(z, pc, 2.48015872894767294178e-05);
    pc = horner(z, pc, -1.38888888888741095749e-03);
    pc = horner(z, pc, 4.16666666666666019037e-02);
    const double cs = std::fma(z * z, pc, std::fma(z, -0.5, 1.0));
    // (the header adds in int; unsigned arithmetic has the same low bits without a signed overflow on the host)
    const int q = (int)(((unsigned)(int)k + (unsigned)kq) & 3u);
    const double a = (q & 1) ? cs : sn, b = (q & 1) ? sn : cs;
    s = (q & 2) ? -a : a;
    c = ((q + 1) & 2) ? -b : b;
}

// ---- the model of the sequences that start from a hardware estimate ----

double rsqrt_fast(double x, double y) {
    const double e = std::fma(-x * y, y, 1.0);
    return std::fma(y, e * std::fma(e, 0.375, 0.5), y);
}

double recip(double x, double y) {
    const double e = std::fma(-x, y, 1.0);
    return std::fma(y, std::fma(e, e, e), y);
}

double sqrt_exact(double x, double y) {
    double g = x * y, h = 0.5 * y;
    const double r = std::fma(-h, g, 0.5);
    g = std::fma(g, r, g);
    h = std::fma(h, r, h);
    double d = std::fma(-g, g, x);
    g = std::fma(d, h, g);
    d = std::fma(-g, g, x);
    return std::fma(d, h, g);
}

uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

template <typename T>
std::vector<T> read_all(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path);
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "short read of %s\n", path);
        exit(2);
    }
    fclose(f);
    return v;
}

FILE *open_out(const char *path) {
    FILE *f = fopen(path, "wb");
    if (!f) {
        fprintf(stderr, "cannot write %s\n", path);
        exit(2);
    }
    return f;
}

template <typename T>
void write_all(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "short write\n");
        exit(2);
    }
}

int usage() {
    fprintf(stderr, "usage: device_math sincos X OUT | sincos_q X KQ OUT | reduce X OUT | "
                    "model sqrt|recip|rsqrt EPS SEED X OUT\n");
    return 2;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return usage();
    const std::string mode = argv[1];
    if (mode == "sincos" || mode == "sincos_q") {
        const bool q = mode == "sincos_q";
        if (argc != (q ? 5 : 4)) return usage();
        const std::vector<double> x = read_all<double>(argv[2]);
        std::vector<int32_t> kq(x.size(), 0);
        if (q) {
            kq = read_all<int32_t>(argv[3]);
            if (kq.size() != x.size()) {
                fprintf(stderr, "%zu arguments, %zu quadrants\n", x.size(), kq.size());
                return 2;
            }
        }
        std::vector<double> s(x.size()), c(x.size());
        for (size_t i = 0; i < x.size(); ++i) {
            if (q)
                sincos_cw_q(x[i], kq[i], s[i], c[i]);
            else
                sincos_cw(x[i], s[i], c[i]);
        }
        FILE *f = open_out(argv[q ? 4 : 3]);
        write_all(f, s);
        write_all(f, c);
        fclose(f);
        return 0;
    }
    if (mode == "reduce") {
        if (argc != 4) return usage();
        const std::vector<double> x = read_all<double>(argv[2]);
        std::vector<double> r(x.size());
        std::vector<int32_t> k(x.size());
        for (size_t i = 0; i < x.size(); ++i) {
            int ki;
            reduce_pio2(x[i], r[i], ki);
            k[i] = ki;
        }
        FILE *f = open_out(argv[3]);
        write_all(f, r);
        write_all(f, k);
        fclose(f);
        return 0;
    }
    if (mode == "model") {
        if (argc != 7) return usage();
        const std::string op = argv[2];
        const double eps = atof(argv[3]);
        uint64_t state = strtoull(argv[4], nullptr, 10);
        const std::vector<double> x = read_all<double>(argv[5]);
        std::vector<double> out(x.size());
        if (op != "sqrt" && op != "recip" && op != "rsqrt") return usage();
        for (size_t i = 0; i < x.size(); ++i) {
            const double u = (i & 3) == 0 ? ((i & 4) ? 1.0 : -1.0)
                                          : 2.0 * (double)(splitmix(state) >> 11) * 0x1p-53 - 1.0;
            const long double exact = op == "recip" ? 1.0L / (long double)x[i] : 1.0L / sqrtl((long double)x[i]);
            const double y = (double)(exact * (1.0L + (long double)u * (long double)eps));
            out[i] = op == "sqrt" ? sqrt_exact(x[i], y) : op == "recip" ? recip(x[i], y) : rsqrt_fast(x[i], y);
        }
        FILE *f = open_out(argv[6]);
        write_all(f, out);
        fclose(f);
        return 0;
    }
    return usage();
}
