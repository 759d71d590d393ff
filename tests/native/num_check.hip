// num_check -- test infrastructure (tests/test_gpu_numerics.py): the device numeric primitives of brent_core.h and
// engine_dev.h, each called alone from a test kernel of a few lines on one block, against host references in long
// double over the inputs their header comments reason about (every PL byte 255 / 0, x = 0.0001 and 0.9999 with 16 full
// slots, table interval boundaries, one-hot lanes) and seeded random ones.  `num_check <section>` runs one section
// (div log wave block quartic poly espoly brent), no argument all of them.  Each prints
//   num_check <section>: N values, M mismatches, max err <measured> (bound <bound>)
// after the first ten offending inputs and indented per-case maxima; exit status 1 on any mismatch, 2 on a HIP error
// (every HIP call is checked; nothing is launched after an error).  The bounds are derived from rounding counts and
// the number formats, never from what the device returns; u = 2^-53 is the unit roundoff throughout.
#include "engine_dev.h"

#include <cinttypes>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#define CK(expr)                                                                                   \
  do {                                                                                             \
    const hipError_t ck_e = (expr);                                                                \
    if (ck_e != hipSuccess) {                                                                      \
      fprintf(stderr, "num_check: %s: %s (line %d)\n", #expr, hipGetErrorString(ck_e), __LINE__); \
      fflush(stdout);                                                                              \
      _Exit(2);                                                                                    \
    }                                                                                              \
  } while (0)

typedef long double ld;
static const ld U53 = 0x1p-53L;

template <class T>
struct Buf {
  T* p = nullptr;
  size_t n;
  explicit Buf(size_t n_) : n(n_) { CK(hipMalloc(&p, sizeof(T) * (n ? n : 1))); CK(hipMemset(p, 0, sizeof(T) * (n ? n : 1))); }
  explicit Buf(const std::vector<T>& v) : n(v.size()) {
    CK(hipMalloc(&p, sizeof(T) * (n ? n : 1)));
    if (n) CK(hipMemcpy(p, v.data(), sizeof(T) * n, hipMemcpyHostToDevice));
  }
  Buf(const Buf&) = delete;
  std::vector<T> get() const {
    std::vector<T> v(n);
    if (n) CK(hipMemcpy(v.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost));
    return v;
  }
  ~Buf() { (void)hipFree(p); }
};
static void ran() { CK(hipGetLastError()); CK(hipDeviceSynchronize()); }

struct Sec {
  const char* name;
  const char* unit;
  ld bound;
  long n = 0, bad = 0;
  ld maxerr = 0;
  void fail(const char* fmt, ...) {
    if (bad++ < 10) {
      va_list ap;
      va_start(ap, fmt);
      printf("  %s: ", name);
      vprintf(fmt, ap);
      printf("\n");
      va_end(ap);
    }
  }
  void err(ld e) { if (e > maxerr) maxerr = e; }
  int done() {
    printf("num_check %s: %ld values, %ld mismatches, max err %.3Lg (bound %.3Lg%s)\n", name, n, bad, maxerr, bound, unit);
    fflush(stdout);
    return bad ? 1 : 0;
  }
};

static uint64_t bits(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
static double from_bits(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }
static double rand_mant(std::mt19937_64& g) { return from_bits(0x3FE0000000000000ull | (g() >> 12)); }   // [0.5, 1)
static double rand_unit(std::mt19937_64& g) { return (double)(g() >> 11) * 0x1p-53; }                      // [0, 1)
static long long ulp_dist(double a, double b) {   // distance of the bit patterns on the ordered line (-0 = +0)
  long long x = (long long)bits(a), y = (long long)bits(b);
  if (x < 0) x = (long long)0x8000000000000000ull - x;
  if (y < 0) y = (long long)0x8000000000000000ull - y;
  return x > y ? x - y : y - x;
}
static ld ulp_of(ld ref) {   // one ulp of the double nearest |ref|
  const double a = fabs((double)ref);
  return (ld)nextafter(a, INFINITY) - (ld)a;
}
// (mantissa in [0.5, 1), exponent) product in long double, renormalised after every factor
struct MantExp {
  ld m = 1.0L;
  long long e = 0;
  void mul(ld f, long long fe = 0) {
    int x;
    m = frexpl(m * f, &x);
    e += (m == 0 ? 0 : x) + fe;
  }
  ld log10() const { return log10l(m) + (ld)e * log10l(2.0L); }
};
// relative error of the device's md 2^ed against a reference pair
static ld rel_err(double md, long long ed, const MantExp& r) {
  if (r.m == 0) return md == 0 ? 0 : INFINITY;
  const long long d = ed - r.e;
  if (d > 200 || d < -200) return INFINITY;
  return fabsl(ldexpl((ld)md, (int)d) - r.m) / r.m;
}

// ---------------------------------------------------------------------------------------------------------- div
__global__ void k_div(const double* n, const double* d, int cnt, double* out) {
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) out[i] = pos_div(n[i], d[i]);
}

static int sec_div() {
  Sec S{"div", " bit-pattern steps from the IEEE quotient", 1};
  std::mt19937_64 rng(0xD1D1);
  std::vector<double> n, d;
  auto rand_normal = [&]() {   // random sign and mantissa, 2^-300 .. 2^300: every quotient stays far inside the normal range
    const double v = ldexp(rand_mant(rng), (int)(rng() % 601) - 300);
    return rng() & 1 ? v : -v;
  };
  auto add = [&](double dd, double paired) {
    n.push_back(0.0); d.push_back(dd);
    n.push_back(paired); d.push_back(dd);
    n.push_back(rand_normal()); d.push_back(dd);
    n.push_back(rand_normal()); d.push_back(dd);
  };
  for (int i = 0; i <= 4097; i++) {   // d = 1 - x on Brent's bracket: both ends and a 4096-point grid
    const double x = i == 0 ? 0.0001 : i == 4097 ? 0.9999 : 0.0001 + (0.9999 - 0.0001) * (i - 1) / 4095.0;
    add(1 - x, x);
  }
  const double s = 0.70710678118654752440;
  for (int i = 0; i < 4096; i++) {   // log10_mant's quotient (m - 1) / (m + 1), m in [sqrt(1/2), sqrt(2))
    const double m = i < 2048 ? s + (2 * s - s) * i / 2048.0 : s + s * rand_unit(rng);
    add(m + 1.0, m - 1.0);
  }
  for (int k = -4; k <= 4; k++) {
    double m = s;
    for (int j = 0; j < (k < 0 ? -k : k); j++) m = nextafter(m, k < 0 ? 0.0 : 2.0);
    add(m + 1.0, m - 1.0);
  }
  for (int k = -500; k <= 500; k++) {   // powers of two and their neighbours
    const double p = ldexp(1.0, k);
    add(p, 1.0);
    add(nextafter(p, 0.0), 1.0);
    add(nextafter(p, INFINITY), rand_mant(rng));
  }
  const int cnt = (int)n.size();
  Buf<double> dn(n), dd(d), dout(cnt);
  k_div<<<1, 1024>>>(dn.p, dd.p, cnt, dout.p);
  ran();
  const std::vector<double> out = dout.get();
  for (int i = 0; i < cnt; i++) {
    const double ref = n[i] / d[i];
    const long long dist = ulp_dist(out[i], ref);
    S.n++;
    S.err((ld)dist);
    if (!(dist <= 1) || std::isnan(out[i])) S.fail("pos_div(%a, %a) = %a, IEEE %a (%lld steps)", n[i], d[i], out[i], ref, dist);
  }
  return S.done();
}

// ---------------------------------------------------------------------------------------------------------- log
__global__ void k_log_mant(const double* m, const int* e, int cnt, double* out) {
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) out[i] = log10_mant(m[i], e[i]);
}
// one (m, e) per wave: lane 0 writes the value, and whether any lane's bits differ from it
__global__ void k_log_u(const double* m, const int* e, int cnt, double* out, int* nonuni) {
  const int w = threadIdx.x >> 6, W = blockDim.x >> 6;
  for (int i = w; i < cnt; i += W) {
    const double r = log10_mant_u(m[i], e[i]);
    const int lo = __double2loint(r), hi = __double2hiint(r);
    const bool diff = lo != __builtin_amdgcn_readfirstlane(lo) || hi != __builtin_amdgcn_readfirstlane(hi);
    const unsigned long long b = __ballot(diff);
    if ((threadIdx.x & 63) == 0) { out[i] = r; nonuni[i] = b != 0; }
  }
}
// two (m, e) per wave, one per half: lanes 0 and 32 write, and whether any lane differs from its half's first
__global__ void k_log_pair(const double* mA, const int* eA, const double* mB, const int* eB, int cnt, double* outA,
                           double* outB, int* nonuni) {
  const int w = threadIdx.x >> 6, W = blockDim.x >> 6, lane = threadIdx.x & 63;
  const bool up = lane >= 32;
  for (int i = w; i < cnt; i += W) {
    const double r = log10_mant_pair(up ? mB[i] : mA[i], up ? eB[i] : eA[i]);
    const int lo = __double2loint(r), hi = __double2hiint(r);
    const int lo0 = __builtin_amdgcn_readlane(lo, 0), hi0 = __builtin_amdgcn_readlane(hi, 0);
    const int lo1 = __builtin_amdgcn_readlane(lo, 32), hi1 = __builtin_amdgcn_readlane(hi, 32);
    const bool diff = up ? (lo != lo1 || hi != hi1) : (lo != lo0 || hi != hi0);
    const unsigned long long b = __ballot(diff);
    if (lane == 0) { outA[i] = r; nonuni[i] = b != 0; }
    if (lane == 32) outB[i] = r;
  }
}

static const int kLogExp[10] = {0, 1, -1, -30, -340, -3400, -34000, -340000, -2000000, 1000};

// the section's bound: 2^-53 (the table form's own error at e = 0: z one rounding, the series, L_i, the last fma) plus
// one ulp of the result (the additions of e log10(2), whose split product is exact to well below that ulp)
static ld log_bound(ld ref) { return U53 + ulp_of(ref); }

static std::vector<double> log_mantissas(std::mt19937_64& rng) {
  std::vector<double> M;
  M.push_back(0.5);
  M.push_back(1 - 0x1p-53);
  for (int i = 0; i <= 128; i++) {   // four doubles on each side of every table interval boundary (1.0: below only)
    const double b = 0.5 + i / 256.0;
    double lo = b, hi = b;
    for (int k = 0; k < 4; k++) {
      lo = nextafter(lo, 0.0);
      if (lo >= 0.5) M.push_back(lo);
      if (hi < 1.0) M.push_back(hi);
      hi = nextafter(hi, 2.0);
    }
  }
  double lo = 0.70710678118654752440, hi = lo;   // log10_mant's branch point
  for (int k = 0; k < 4; k++) { M.push_back(hi); hi = nextafter(hi, 2.0); lo = nextafter(lo, 0.0); M.push_back(lo); }
  for (int i = 0; i < 20000; i++) M.push_back(rand_mant(rng));
  return M;
}

static int sec_log() {
  Sec S{"log", " of each value's bound 2^-53 + ulp(|reference|)", 1};
  std::mt19937_64 rng(0x106);
  const std::vector<double> M = log_mantissas(rng);
  const int nm = (int)M.size(), cnt = nm * 10 + 10;
  std::vector<double> m(cnt);
  std::vector<int> e(cnt);
  for (int i = 0; i < nm; i++)
    for (int k = 0; k < 10; k++) { m[i * 10 + k] = M[i]; e[i * 10 + k] = kLogExp[k]; }
  for (int k = 0; k < 10; k++) { m[nm * 10 + k] = 0.0; e[nm * 10 + k] = kLogExp[k]; }   // m == 0: -inf
  Buf<double> dm(m), dout(cnt), dou(cnt);
  Buf<int> de(e), dnon(cnt);
  k_log_mant<<<1, 1024>>>(dm.p, de.p, cnt, dout.p);
  ran();
  k_log_u<<<1, 1024>>>(dm.p, de.p, cnt, dou.p, dnon.p);
  ran();
  const std::vector<double> om = dout.get(), ou = dou.get();
  const std::vector<int> non = dnon.get();
  ld worst[2][10] = {};
  for (int i = 0; i < cnt; i++) {
    const int k = i % 10;
    for (int f = 0; f < 2; f++) {
      const double got = f ? ou[i] : om[i];
      const char* fn = f ? "log10_mant_u" : "log10_mant";
      S.n++;
      if (m[i] == 0.0) {
        if (!(std::isinf(got) && got < 0)) S.fail("%s(0, %d) = %a, not -inf", fn, e[i], got);
        continue;
      }
      const ld ref = log10l((ld)m[i]) + (ld)e[i] * log10l(2.0L);
      const ld err = fabsl((ld)got - ref), bound = log_bound(ref);
      if (err > worst[f][k]) worst[f][k] = err;
      S.err(err / bound);
      if (!(err <= bound)) S.fail("%s(%a, %d) = %.17g, reference %.21Lg: error %.3Lg > %.3Lg", fn, m[i], e[i], got, ref, err, bound);
    }
    if (non[i]) S.fail("log10_mant_u(%a, %d): the 64 lanes do not hold the same bits", m[i], e[i]);
  }
  for (int f = 0; f < 2; f++)
    for (int k = 0; k < 10; k++)
      printf("  %-12s e = %8d: max abs error %.3Lg\n", f ? "log10_mant_u" : "log10_mant", kLogExp[k], worst[f][k]);

  // pairs: the two halves take values from different table intervals (a fixed stride through the list), neighbours
  // across a boundary, and zero next to a non-zero; each half must equal log10_mant_u of its own value bit for bit
  std::vector<int> ia, ib;
  for (int i = 0; i < cnt; i++) { ia.push_back(i); ib.push_back((int)(((long long)i * 7919 + 4321) % cnt)); }
  for (int i = 0; i + 10 < cnt; i++) { ia.push_back(i); ib.push_back(i + 10); }
  for (int k = 0; k < 10; k++) { ia.push_back(nm * 10 + k); ib.push_back(k * 977 % (nm * 10)); ia.push_back(k * 1013 % (nm * 10)); ib.push_back(nm * 10 + k); }
  const int np = (int)ia.size();
  std::vector<double> mA(np), mB(np);
  std::vector<int> eA(np), eB(np);
  for (int p = 0; p < np; p++) { mA[p] = m[ia[p]]; eA[p] = e[ia[p]]; mB[p] = m[ib[p]]; eB[p] = e[ib[p]]; }
  Buf<double> dmA(mA), dmB(mB), doA(np), doB(np);
  Buf<int> deA(eA), deB(eB), dnp(np);
  k_log_pair<<<1, 1024>>>(dmA.p, deA.p, dmB.p, deB.p, np, doA.p, doB.p, dnp.p);
  ran();
  const std::vector<double> oA = doA.get(), oB = doB.get();
  const std::vector<int> nonp = dnp.get();
  for (int p = 0; p < np; p++) {
    S.n += 2;
    if (bits(oA[p]) != bits(ou[ia[p]]))
      S.fail("log10_mant_pair low half (%a, %d) [high half %a] = %a, log10_mant_u %a", mA[p], eA[p], mB[p], oA[p], ou[ia[p]]);
    if (bits(oB[p]) != bits(ou[ib[p]]))
      S.fail("log10_mant_pair high half (%a, %d) [low half %a] = %a, log10_mant_u %a", mB[p], eB[p], mA[p], oB[p], ou[ib[p]]);
    if (nonp[p]) S.fail("log10_mant_pair(%a | %a): a half's lanes do not hold the same bits", mA[p], mB[p]);
  }
  return S.done();
}

// ---------------------------------------------------------------------------------------------------------- wave
template <bool PAIR>
__global__ void k_wave(const double* m, const int* e, int ncase, double* om, int* oe) {
  const int w = threadIdx.x >> 6, W = blockDim.x >> 6, lane = threadIdx.x & 63;
  for (int c = w; c < ncase; c += W) {
    double mm = m[c * 64 + lane];
    int ee = e[c * 64 + lane];
    if (PAIR) wave_prod_pair(mm, ee); else wave_prod(mm, ee);
    om[c * 64 + lane] = mm;
    oe[c * 64 + lane] = ee;
  }
}
__global__ void k_wsum(const double* v, int ncase, double* out) {
  const int w = threadIdx.x >> 6, W = blockDim.x >> 6, lane = threadIdx.x & 63;
  for (int c = w; c < ncase; c += W) out[c * 64 + lane] = wave_sum_exact(v[c * 64 + lane]);
}

// per-lane mantissas in [1/16, 1) (what lane_poly_r hands over) and arbitrary exponents
static void wave_cases(std::mt19937_64& rng, std::vector<double>& m, std::vector<int>& e) {
  auto add = [&](auto f) {
    for (int l = 0; l < 64; l++) {
      double mm; int ee;
      f(l, mm, ee);
      m.push_back(mm); e.push_back(ee);
    }
  };
  for (int k = 0; k < 64; k++)   // one-hot: lane k holds 0.75 x 2^(k+1), the others 1.0 as 1/2 x 2^1
    add([&](int l, double& mm, int& ee) { mm = l == k ? 0.75 : 0.5; ee = l == k ? k + 1 : 1; });
  add([&](int, double& mm, int& ee) { mm = 1.0 / 16; ee = 0; });            // the product 2^-256 of the header comment
  add([&](int l, double& mm, int& ee) { mm = 1.0 / 16; ee = 3 * l - 7; });
  add([&](int, double& mm, int& ee) { mm = 1 - 0x1p-53; ee = 0; });
  add([&](int l, double& mm, int& ee) { mm = l == 37 ? 0.0 : 0.625; ee = l; });   // one lane at 0
  add([&](int l, double& mm, int& ee) { mm = l == 5 ? 0.0 : 0.625; ee = -l; });   // (the other half)
  for (int c = 0; c < 1000; c++) {
    const int span = c % 3 == 0 ? 1 << 25 : c % 3 == 1 ? 2000000 : 40;   // 64 x 2^25 stays an int
    add([&](int, double& mm, int& ee) {
      mm = ldexp(rand_mant(rng), -(int)(rng() % 4));
      ee = (int)(rng() % (2 * span + 1)) - span;
    });
  }
}

static int sec_wave() {
  Sec S{"wave", " x 2^-53 relative", 64};   // 63 multiplies of <= 2^-53 each (first order), scalings exact
  std::mt19937_64 rng(0x3A7E);
  std::vector<double> m;
  std::vector<int> e;
  wave_cases(rng, m, e);
  const int nc = (int)m.size() / 64;
  Buf<double> dm(m), dom(m.size());
  Buf<int> de(e), doe(e.size());
  const ld bound = powl(1 + U53, 63) - 1;
  for (int pair = 0; pair < 2; pair++) {
    if (pair) k_wave<true><<<1, 1024>>>(dm.p, de.p, nc, dom.p, doe.p);
    else k_wave<false><<<1, 1024>>>(dm.p, de.p, nc, dom.p, doe.p);
    ran();
    const std::vector<double> om = dom.get();
    const std::vector<int> oe = doe.get();
    const char* fn = pair ? "wave_prod_pair" : "wave_prod";
    for (int c = 0; c < nc; c++)
      for (int h = 0; h < (pair ? 2 : 1); h++) {
        const int l0 = c * 64 + h * 32, nl = pair ? 32 : 64;
        MantExp ref;
        for (int l = 0; l < nl; l++) ref.mul((ld)m[l0 + l], e[l0 + l]);
        S.n++;
        bool uni = true;
        for (int l = 1; l < nl; l++) uni = uni && bits(om[l0 + l]) == bits(om[l0]) && (om[l0] == 0 || oe[l0 + l] == oe[l0]);
        if (!uni) { S.fail("%s case %d half %d: lanes differ", fn, c, h); continue; }
        const double md = om[l0];
        if (!(md == 0 || (md >= 0.5 && md < 1))) { S.fail("%s case %d half %d: mantissa %a outside [0.5, 1)", fn, c, h, md); continue; }
        const ld err = rel_err(md, oe[l0], ref);
        S.err(err / U53);
        if (!(err <= bound))
          S.fail("%s case %d half %d: %a x 2^%d, reference %.21Lg x 2^%lld (relative error %.3Lg)", fn, c, h, md, oe[l0], ref.m, ref.e, err);
      }
  }
  // wave_sum_exact: integers below 2^46 per lane (sum < 2^52) add without rounding, identically in every lane
  std::vector<double> v;
  std::vector<long long> want;
  for (int c = 0; c < 64 + 200; c++) {
    long long s = 0;
    for (int l = 0; l < 64; l++) {
      const long long x = c < 64 ? (l == c ? (1ll << 45) + 12345 + c : 0) : (long long)(rng() >> 18);
      v.push_back((double)x);
      s += x;
    }
    want.push_back(s);
  }
  Buf<double> dv(v), dsum(v.size());
  k_wsum<<<1, 1024>>>(dv.p, (int)want.size(), dsum.p);
  ran();
  const std::vector<double> sum = dsum.get();
  for (size_t c = 0; c < want.size(); c++) {
    S.n++;
    for (int l = 0; l < 64; l++)
      if (sum[c * 64 + l] != (double)want[c]) { S.fail("wave_sum_exact case %zu lane %d: %.17g, exact %lld", c, l, sum[c * 64 + l], want[c]); break; }
  }
  return S.done();
}

// ---------------------------------------------------------------------------------------------------------- block
#define BLK_CALLS 8
// as k_brent uses it: consecutive calls on the toggling double buffer, no barrier of the caller's between them
template <int T>
__global__ void __launch_bounds__(T) k_block(const double* m, const int* e, double* out) {
  __shared__ double s_red[32];
  __shared__ int s_rede[32];
  int par = 0;
  double mm[BLK_CALLS], r[BLK_CALLS];
  int ee[BLK_CALLS];
#pragma unroll
  for (int c = 0; c < BLK_CALLS; c++) { mm[c] = m[c * T + threadIdx.x]; ee[c] = e[c * T + threadIdx.x]; }
#pragma unroll
  for (int c = 0; c < BLK_CALLS; c++) r[c] = block_logprod<T>(mm[c], ee[c], s_red, s_rede, par);   // back to back, from registers
#pragma unroll
  for (int c = 0; c < BLK_CALLS; c++) out[c * T + threadIdx.x] = r[c];
}

template <int T>
static void block_T(Sec& S, std::mt19937_64& rng) {
  constexpr int W = T / 64, NSET = 12, N = BLK_CALLS * T;
  // T multiplies inside the waves and T/64 across them, each <= 2^-53 relative, as an absolute error of the log10;
  // then the table log10 itself (the log section's bound)
  const ld prod_bound = (ld)(T + W) * U53 / logl(10.0L);
  ld worst = 0;
  for (int set = 0; set < NSET; set++) {
    std::vector<double> m(N);
    std::vector<int> e(N);
    for (int c = 0; c < BLK_CALLS; c++)
      for (int t = 0; t < T; t++) {
        double mm = 0.5; int ee = 1;
        if (set == 0) {   // one-hot over waves: one lane of wave c mod W holds 0.75 x 2^(c+2)
          if (t == (c % W) * 64 + (17 * c + 5) % 64) { mm = 0.75; ee = c + 2; }
        } else if (set == 1) {   // every factor 1/16: 2^(-4 T)
          mm = 1.0 / 16; ee = 0;
        } else if (set == 2) {   // one factor 0 in every second call: -inf, then finite again
          mm = (c & 1) && t == (31 * c) % T ? 0.0 : 0.75; ee = c;
        } else {
          mm = ldexp(rand_mant(rng), -(int)(rng() % 4));
          const int span = set % 3 == 0 ? 2 : set % 3 == 1 ? 1000 : 30;
          ee = (int)(rng() % (2 * span + 1)) - span;
        }
        m[c * T + t] = mm; e[c * T + t] = ee;
      }
    Buf<double> dm(m), dout(N);
    Buf<int> de(e);
    k_block<T><<<1, T>>>(dm.p, de.p, dout.p);
    ran();
    const std::vector<double> out = dout.get();
    for (int c = 0; c < BLK_CALLS; c++) {
      MantExp ref;
      for (int t = 0; t < T; t++) ref.mul((ld)m[c * T + t], e[c * T + t]);
      for (int t = 0; t < T; t++) {
        const double got = out[c * T + t];
        S.n++;
        if (ref.m == 0) {
          if (!(std::isinf(got) && got < 0)) S.fail("block_logprod<%d> set %d call %d thread %d: %a, not -inf", T, set, c, t, got);
          continue;
        }
        const ld r = ref.log10(), err = fabsl((ld)got - r), bound = prod_bound + log_bound(r);
        S.err(err / bound);
        if (err > worst) worst = err;
        if (!(err <= bound))
          S.fail("block_logprod<%d> set %d call %d thread %d: %.17g, reference %.21Lg (error %.3Lg > %.3Lg)", T, set, c, t, got, r, err, bound);
      }
    }
  }
  printf("  block_logprod<%4d>: max abs error %.3Lg (product part of the bound %.3Lg)\n", T, worst, prod_bound);
}

static int sec_block() {
  Sec S{"block", " of each value's bound (T + T/64) 2^-53 / ln 10 + 2^-53 + ulp(|reference|)", 1};
  std::mt19937_64 rng(0xB10C);
  block_T<64>(S, rng);
  block_T<128>(S, rng);
  block_T<256>(S, rng);
  block_T<512>(S, rng);
  block_T<1024>(S, rng);
  return S.done();
}

// ---------------------------------------------------------------------------------------------------------- quartic
struct Fam {
  uint32_t by[12];   // by[3 q + k]: PL byte of person q (father, mother, kids) for genotype k (11, 12, 22)
  int nn;            // persons: 0 (empty slot), 2, 3, 4
};
// V: 0 fam_poly4<0,false>  1 <3,false>  2 <4,false>  3 <0,true>  4 <3,true>
//    5 the nine-product form: likelihoodONEKid per parental pair (d_one_kid), c9, fold_poly   6 quad_poly4 called directly
template <int V>
__global__ void k_quartic(const Fam* fam, int cnt, const double* lk, double* out) {
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    uint32_t by[12];
    for (int j = 0; j < 12; j++) by[j] = fam[i].by[j];
    const int nn = fam[i].nn;
    double a[5];
    if constexpr (V == 0) fam_poly4<0, false>(by, nn, lk, a);
    if constexpr (V == 1) fam_poly4<3, false>(by, nn, lk, a);
    if constexpr (V == 2) fam_poly4<4, false>(by, nn, lk, a);
    if constexpr (V == 3) fam_poly4<0, true>(by, nn, lk, a);
    if constexpr (V == 4) fam_poly4<3, true>(by, nn, lk, a);
    if constexpr (V == 5) {
      double c9[9];
      for (int k = 0; k < 9; k++) {
        double kids = 1.0;
        for (int q = 2; q < nn; q++) kids *= d_one_kid(k, PM_CHR_AUTO, 0, lk[by[3 * q]], lk[by[3 * q + 1]], lk[by[3 * q + 2]]);
        c9[k] = kids * (lk[by[k / 3]] * lk[by[3 + k % 3]]);
      }
      fold_poly(c9, a);
    }
    if constexpr (V == 6) {
      double D[2][3];
      for (int q = 0; q < 2; q++)
        for (int k = 0; k < 3; k++) D[q][k] = 2 + q < nn ? lk[by[3 * (2 + q) + k]] : 1.0;
      const double lF[3] = {lk[by[0]], lk[by[1]], lk[by[2]]}, lM[3] = {lk[by[3]], lk[by[4]], lk[by[5]]};
      quad_poly4(D, lF, lM, a);
    }
    for (int j = 0; j < 5; j++) out[i * 5 + j] = a[j];
  }
}

// P(kid genotype g | father x, mother y), autosomal, genotypes (11, 12, 22); row 3 x + y
static const ld kMendel[9][3] = {
    {1, 0, 0},           // 11 x 11
    {0.5L, 0.5L, 0},     // 11 x 12
    {0, 1, 0},           // 11 x 22
    {0.5L, 0.5L, 0},     // 12 x 11
    {0.25L, 0.5L, 0.25L},// 12 x 12
    {0, 0.5L, 0.5L},     // 12 x 22
    {0, 1, 0},           // 22 x 11
    {0, 0.5L, 0.5L},     // 22 x 12
    {0, 0, 1},           // 22 x 22
};
static void ref_quartic(const Fam& F, const double* lk, ld* a) {
  if (F.nn == 0) { a[0] = 1; a[1] = 4; a[2] = 6; a[3] = 4; a[4] = 1; return; }
  ld c[9];
  for (int x = 0; x < 3; x++)
    for (int y = 0; y < 3; y++) {
      ld v = (ld)lk[F.by[x]] * (ld)lk[F.by[3 + y]];
      for (int q = 2; q < F.nn; q++) {
        ld s = 0;
        for (int g = 0; g < 3; g++) s += kMendel[3 * x + y][g] * (ld)lk[F.by[3 * q + g]];
        v *= s;
      }
      c[3 * x + y] = v;
    }
  a[0] = c[0]; a[1] = 2 * (c[1] + c[3]); a[2] = c[2] + 4 * c[4] + c[6]; a[3] = 2 * (c[5] + c[7]); a[4] = c[8];
}

static void host_lk(double* lk) {
  for (int i = 0; i <= 255; i++) lk[i] = pow(0.1, i * 0.1);   // the engine's table (host glibc)
}

// PL bytes per person: all 0, all 255, one 0 among 255s in each position, random
static std::vector<Fam> quartic_fams(std::mt19937_64& rng, const std::vector<int>& nns, int nrand) {
  std::vector<Fam> F;
  for (int nn : nns) {
    for (int pat = 0; pat < 5 + nrand; pat++) {
      Fam f;
      f.nn = nn;
      for (int q = 0; q < 4; q++)
        for (int k = 0; k < 3; k++)
          f.by[3 * q + k] = pat == 0 ? 0 : pat == 1 ? 255 : pat < 5 ? (k == pat - 2 ? 0 : 255)
                            : pat % 4 == 1 ? (rng() % 3 ? 255 : 0) : pat % 4 == 2 ? (uint32_t)(rng() % 3 == 0 ? 0 : rng() % 256) : (uint32_t)(rng() % 256);
      F.push_back(f);
      if (nn == 0) break;   // an empty slot: one case with zero bytes, and below one with random ones
    }
    if (nn == 0) {
      Fam f;
      f.nn = 0;
      for (int j = 0; j < 12; j++) f.by[j] = (uint32_t)(rng() % 256);
      F.push_back(f);
    }
  }
  return F;
}

template <int V>
static std::vector<double> run_quartic(const std::vector<Fam>& F, const double* lk) {
  Buf<Fam> dF(F);
  Buf<double> dlk(std::vector<double>(lk, lk + 256)), dout(F.size() * 5);
  k_quartic<V><<<1, 256>>>(dF.p, (int)F.size(), dlk.p, dout.p);
  ran();
  return dout.get();
}

// Roundings of quad_poly4's longest chain, a[2] = fma(P2, s02, (0.25 PC) (lF1 lM1)), every term non-negative:
//   Ct[q] = fma(2, D1, D0) + D2       2   (per kid)
//   PC = Ct[0] Ct[1]                  2 + 2 + 1 = 5
//   0.25 PC                           exact
//   lF1 lM1                           1
//   (0.25 PC) (lF1 lM1)               5 + 1 + 1 = 7
//   P2 s02 inside the fma             P2: 1, s02 = fma(., ., one product): 2 -> 3, not rounded itself
//   the fma's sum                     max(7, 3) + 1 = 8
// so every coefficient is within (1 + u)^8 - 1 of its real value.  (The nine-product form's a[2] = c2 + 4 c4 + c6
// counts 9, so the two forms can differ by 17 in the worst case; the check holds them to twice 8 all the same.)
static const int kQuarticRoundings = 8;

template <int V>
static void quartic_variant(Sec& S, const char* fn, const std::vector<Fam>& F, const double* lk, std::vector<double>* keep = nullptr) {
  const std::vector<double> out = run_quartic<V>(F, lk);
  const ld bound = powl(1 + U53, kQuarticRoundings) - 1;
  ld worst = 0;
  for (size_t i = 0; i < F.size(); i++) {
    ld ref[5];
    ref_quartic(F[i], lk, ref);
    for (int j = 0; j < 5; j++) {
      const double got = out[i * 5 + j];
      S.n++;
      if (F[i].nn == 0) {
        if (got != (double)ref[j]) S.fail("%s family %zu (empty slot) a[%d] = %a, not %Lg", fn, i, j, got, ref[j]);
        continue;
      }
      if (!(std::isfinite(got) && got > 0)) { S.fail("%s family %zu (nn %d) a[%d] = %a: not finite and positive", fn, i, F[i].nn, j, got); continue; }
      const ld err = fabsl((ld)got - ref[j]) / ref[j];
      if (err > worst) worst = err;
      S.err(err / U53);
      if (!(err <= bound))
        S.fail("%s family %zu (nn %d, bytes %u %u %u | %u %u %u | %u %u %u | %u %u %u) a[%d] = %a, reference %.21Lg (%.2Lf x 2^-53)", fn, i,
               F[i].nn, F[i].by[0], F[i].by[1], F[i].by[2], F[i].by[3], F[i].by[4], F[i].by[5], F[i].by[6], F[i].by[7], F[i].by[8],
               F[i].by[9], F[i].by[10], F[i].by[11], j, got, ref[j], err / U53);
    }
  }
  printf("  %-28s max relative error %.2Lf x 2^-53\n", fn, worst / U53);
  if (keep) *keep = out;
}

static int sec_quartic() {
  Sec S{"quartic", " x 2^-53 relative", (ld)kQuarticRoundings};
  std::mt19937_64 rng(0x9A27);
  double lk[256];
  host_lk(lk);
  const int NR = 1500;
  const std::vector<Fam> any = quartic_fams(rng, {0, 2, 3, 4}, NR), trio = quartic_fams(rng, {0, 3}, NR),
                         quad = quartic_fams(rng, {0, 4}, NR), rquad = quartic_fams(rng, {4}, NR), rtrio = quartic_fams(rng, {3}, NR);
  std::vector<double> fact, nine;
  quartic_variant<0>(S, "fam_poly4<0,false>", any, lk, &fact);
  quartic_variant<1>(S, "fam_poly4<3,false>", trio, lk);
  quartic_variant<2>(S, "fam_poly4<4,false>", quad, lk);
  quartic_variant<3>(S, "fam_poly4<0,true>", rquad, lk);
  quartic_variant<4>(S, "fam_poly4<3,true>", rtrio, lk);
  std::vector<Fam> real;   // the forms without the empty-slot select: real families only
  std::vector<size_t> at;
  for (size_t i = 0; i < any.size(); i++)
    if (any[i].nn) { real.push_back(any[i]); at.push_back(i); }
  quartic_variant<5>(S, "d_one_kid products, fold_poly", real, lk, &nine);
  quartic_variant<6>(S, "quad_poly4", real, lk);
  ld worst = 0;
  const ld bound2 = 2 * (powl(1 + U53, kQuarticRoundings) - 1);
  for (size_t r = 0; r < real.size(); r++)
    for (int j = 0; j < 5; j++) {
      const double f = fact[at[r] * 5 + j], n = nine[r * 5 + j];
      S.n++;
      const ld d = fabsl((ld)f - (ld)n) / fminl((ld)f, (ld)n);
      if (d > worst) worst = d;
      if (!(d <= bound2)) S.fail("family %zu a[%d]: factored %a, nine products %a (%.2Lf x 2^-53 apart)", at[r], j, f, n, d / U53);
    }
  printf("  factored against nine products: at most %.2Lf x 2^-53 apart (bound %d)\n", worst / U53, 2 * kQuarticRoundings);
  return S.done();
}

// ---------------------------------------------------------------------------------------------------------- poly
// as the engine calls them: r = pos_div(x, g), g4 = (g g)(g g); the r handed over is written out for the reference
template <int S, int NC>
__global__ void k_poly(const double* coef, const double* m0, const int* e0, const double* x, const int* pat, int cnt, double* om,
                       int* oe, double* otm, int* ote, double* orr) {
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    const int p = pat[i];
    double a[S][NC];
    for (int s = 0; s < S; s++)
      for (int k = 0; k < NC; k++) a[s][k] = coef[((size_t)p * S + s) * NC + k];
    const double xx = x[i], g = 1 - xx;
    const double r = pos_div(xx, g);
    double m, tm;
    int e, te;
    lane_poly_r<S, NC>(r, (g * g) * (g * g), (const double(*)[NC])a, m, e, m0[p], e0[p]);
    lane_poly_top<S, NC>((const double(*)[NC])a, tm, te, m0[p], e0[p]);
    om[i] = m; oe[i] = e; otm[i] = tm; ote[i] = te; orr[i] = r;
  }
}

// Roundings of lane_poly_r<S> (PM_G4_LATE) against m0 2^e0 prod_s g^4 h_s(r) at the same doubles r, g and coefficients:
//   h_s: four fma on non-negative terms          4 each                        4 S
//   the accumulators' multiplies by h_s          1 each                        S
//   the accumulator tree                         min(S, 4) - 1
//   g4 = (g g)(g g)                              3, to the power S             3 S
//   (g4)^S by squaring                           S - 1 multiplies' weight      S - 1
//   m p                                          1
// 9 S + min(S, 4) - 1 in all: 9, 19, 39, 75, 147 for S = 1 .. 16, below the 12 S of the header's "<= ~8 ulp" per
// family with g4, the product and the renormalisation added; frexp and the exponent sums are exact.
static int poly_roundings(int S) { return 9 * S + (S < 4 ? S : 4) - 1; }
// lane_poly_top<S>: S multiplies by a[s][0] (the first by the seed) and the tree
static int top_roundings(int S) { return S + (S < 4 ? S : 4) - 1; }

template <int S, int NC>
static void poly_SN(Sec& Sx, const std::vector<std::vector<double>>& famc, std::mt19937_64& rng) {
  // famc: 0 all-255 quad, 1 all-0 quad, 2 phantom, 3.. other families (five coefficients each)
  const int nf = (int)famc.size();
  std::vector<std::vector<int>> pats;
  auto pat = [&](auto f) { std::vector<int> v(S); for (int s = 0; s < S; s++) v[s] = f(s); pats.push_back(v); };
  pat([](int) { return 0; });                  // all-255 families in every slot
  pat([](int) { return 1; });                  // all-0 families
  pat([](int s) { return s & 1; });            // the two alternating
  pat([](int s) { return 1 - (s & 1); });
  pat([](int s) { return s & 1 ? 2 : 0; });    // phantom slots mixed in
  pat([](int s) { return s % 3 == 0 ? 2 : 0; });
  pat([](int) { return 2; });
  for (int k = 0; k < 10; k++) pat([&](int) { return rng() % 4 == 0 ? 2 : 3 + (int)(rng() % (nf - 3)); });
  const int np = (int)pats.size();
  std::vector<double> coef((size_t)np * S * NC), m0(np, 1.0);
  std::vector<int> e0(np, 0);
  for (int p = 0; p < np; p++)
    for (int s = 0; s < S; s++) {
      const std::vector<double>& a = famc[pats[p][s]];
      double* c = &coef[((size_t)p * S + s) * NC];
      if (NC == 5) for (int k = 0; k < 5; k++) c[k] = a[k];
      else {   // b_k = a_k / a4 and the normalised product of the a4, in double: the kernel's and the reference's inputs
        for (int k = 0; k < 4; k++) c[k] = a[k] / a[4];
        int x;
        m0[p] = frexp(m0[p] * a[4], &x);
        e0[p] += x;
      }
    }
  std::vector<double> xs = {0.0001, 0.5, 0.9999};
  for (int i = 1; i <= 33; i++) xs.push_back(0.0001 + (0.9999 - 0.0001) * i / 34.0);
  std::vector<double> x;
  std::vector<int> pi;
  for (int p = 0; p < np; p++)
    for (double v : xs) { x.push_back(v); pi.push_back(p); }
  const int cnt = (int)x.size();
  Buf<double> dc(coef), dm0(m0), dx(x), dom(cnt), dotm(cnt), dorr(cnt);
  Buf<int> de0(e0), dp(pi), doe(cnt), dote(cnt);
  k_poly<S, NC><<<1, 256>>>(dc.p, dm0.p, de0.p, dx.p, dp.p, cnt, dom.p, doe.p, dotm.p, dote.p, dorr.p);
  ran();
  const std::vector<double> om = dom.get(), otm = dotm.get(), orr = dorr.get();
  const std::vector<int> oe = doe.get(), ote = dote.get();
  const ld bound = powl(1 + U53, poly_roundings(S)) - 1, tbound = powl(1 + U53, top_roundings(S)) - 1;
  ld worst = 0, tworst = 0;
  for (int i = 0; i < cnt; i++) {
    const int p = pi[i];
    const ld g = (ld)(1 - x[i]), r = (ld)orr[i], g4 = (g * g) * (g * g);
    MantExp ref, top;
    ref.mul((ld)m0[p], e0[p]);
    top.mul((ld)m0[p], e0[p]);
    for (int s = 0; s < S; s++) {
      const double* c = &coef[((size_t)p * S + s) * NC];
      const ld last = NC == 4 ? 1.0L : (ld)c[NC - 1];
      ref.mul(g4);
      ref.mul((((c[0] * r + c[1]) * r + c[2]) * r + c[3]) * r + last);
      top.mul((ld)c[0]);
    }
    Sx.n += 2;
    if (ulp_dist(orr[i], x[i] / (1 - x[i])) > 1) Sx.fail("S %d NC %d x %.17g: r = %a is not within an ulp of x / g", S, NC, x[i], orr[i]);
    if (!(std::isfinite(om[i]) && om[i] >= 1.0 / 16 && om[i] < 1)) {
      Sx.fail("lane_poly_r<%d,%d> pattern %d x %.17g: mantissa %a outside [1/16, 1)", S, NC, p, x[i], om[i]);
    } else {
      const ld err = rel_err(om[i], oe[i], ref);
      if (err > worst) worst = err;
      Sx.err(err / bound);
      if (!(err <= bound))
        Sx.fail("lane_poly_r<%d,%d> pattern %d x %.17g: %a x 2^%d, reference %.21Lg x 2^%lld (%.2Lf x 2^-53 > %d)", S, NC, p, x[i], om[i],
                oe[i], ref.m, ref.e, err / U53, poly_roundings(S));
    }
    if (!(std::isfinite(otm[i]) && otm[i] >= 1.0 / 16 && otm[i] < 1)) {
      Sx.fail("lane_poly_top<%d,%d> pattern %d: mantissa %a outside [1/16, 1)", S, NC, p, otm[i]);
    } else {
      const ld err = rel_err(otm[i], ote[i], top);
      if (err > tworst) tworst = err;
      Sx.err(err / tbound);
      if (!(err <= tbound))
        Sx.fail("lane_poly_top<%d,%d> pattern %d: %a x 2^%d, reference %.21Lg x 2^%lld (%.2Lf x 2^-53)", S, NC, p, otm[i], ote[i], top.m,
                top.e, err / U53);
    }
  }
  printf("  S %2d NC %d: lane_poly_r %.2Lf x 2^-53 (bound %d), lane_poly_top %.2Lf x 2^-53 (bound %d)\n", S, NC, worst / U53,
         poly_roundings(S), tworst / U53, top_roundings(S));
}

static int sec_poly() {
  Sec S{"poly", " of each value's bound (9 S + min(S, 4) - 1) 2^-53, lane_poly_top (S + min(S, 4) - 1) 2^-53", 1};
  std::mt19937_64 rng(0x9017);
  double lk[256];
  host_lk(lk);
  std::vector<Fam> F = quartic_fams(rng, {4}, 40);   // [0] all 0, [1] all 255, then one-zero and random quads
  const std::vector<Fam> more = quartic_fams(rng, {3, 2}, 12);
  F.insert(F.end(), more.begin(), more.end());
  const std::vector<double> a = run_quartic<0>(F, lk);   // the quartic section's coefficients, from the device
  std::vector<std::vector<double>> famc;
  auto fam = [&](size_t i) { return std::vector<double>(a.begin() + i * 5, a.begin() + i * 5 + 5); };
  famc.push_back(fam(1));
  famc.push_back(fam(0));
  famc.push_back({1.0, 4.0, 6.0, 4.0, 1.0});
  for (size_t i = 2; i < F.size(); i++) famc.push_back(fam(i));
  for (const std::vector<double>& c : famc)
    for (double v : c)
      if (!(std::isfinite(v) && v > 0)) { S.fail("a coefficient from fam_poly4 is %a", v); return S.done(); }
  poly_SN<1, 5>(S, famc, rng); poly_SN<1, 4>(S, famc, rng);
  poly_SN<2, 5>(S, famc, rng); poly_SN<2, 4>(S, famc, rng);
  poly_SN<4, 5>(S, famc, rng); poly_SN<4, 4>(S, famc, rng);
  poly_SN<8, 5>(S, famc, rng); poly_SN<8, 4>(S, famc, rng);
  poly_SN<16, 5>(S, famc, rng); poly_SN<16, 4>(S, famc, rng);
  return S.done();
}

// ---------------------------------------------------------------------------------------------------------- espoly
#define ESP_MAX 13
// coefficient a of item i at c[a * cnt + i] (the engine's lane-strided layout); out: es_poly_eval, _r<8>, _r<12>
__global__ void k_espoly(const double* c, const int* D, const double* x, int cnt, double* out) {
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    double r[ESP_MAX];
    for (int a = 0; a < ESP_MAX; a++) r[a] = c[(size_t)a * cnt + i];
    out[i] = es_poly_eval(c + i, (size_t)cnt, D[i], x[i]);
    out[cnt + i] = D[i] <= 8 ? es_poly_eval_r<8>(r, D[i], x[i]) : 0.0;
    out[2 * cnt + i] = es_poly_eval_r<12>(r, D[i], x[i]);
  }
}

static int sec_espoly() {
  Sec S{"espoly", " of each value's bound (3 D + 4) 2^-53 relative", 1};
  std::mt19937_64 rng(0xE5);
  const int Ds[5] = {0, 1, 4, 8, 12};
  const double xs[6] = {0.0001, 0.25, 0.5, nextafter(0.5, 1.0), 0.75, 0.9999};
  std::vector<std::vector<double>> cs;
  std::vector<int> D;
  std::vector<double> x;
  for (int d : Ds)
    for (double xv : xs)
      for (int rep = 0; rep < 200; rep++) {
        std::vector<double> c(ESP_MAX, 0.0);
        for (int a = 0; a <= d; a++)   // non-negative, across 1e-200 .. 1 (rep 0: all equal, rep 1: some exactly 0)
          c[a] = rep == 0 ? 0.375 : (rep % 8 == 1 && rng() % 3 == 0) ? 0.0 : pow(10.0, -200.0 * rand_unit(rng) * (rep % 2 ? 1.0 : 0.02));
        cs.push_back(c); D.push_back(d); x.push_back(xv);
      }
  const int cnt = (int)D.size();
  std::vector<double> flat((size_t)ESP_MAX * cnt);
  for (int i = 0; i < cnt; i++)
    for (int a = 0; a < ESP_MAX; a++) flat[(size_t)a * cnt + i] = cs[i][a];
  Buf<double> dc(flat), dx(x), dout((size_t)3 * cnt);
  Buf<int> dD(D);
  k_espoly<<<1, 256>>>(dc.p, dD.p, dx.p, cnt, dout.p);
  ran();
  const std::vector<double> out = dout.get();
  ld worst[ESP_MAX] = {};
  for (int i = 0; i < cnt; i++) {
    // L = sum_a c_a x^a g^(D - a) with g the double 1 - x the functions form (exact for four of the six x)
    const ld g = (ld)(1 - x[i]), xl = (ld)x[i];
    ld ref = 0;
    for (int a = 0; a <= D[i]; a++) ref += (ld)cs[i][a] * powl(xl, a) * powl(g, D[i] - a);
    const double got = out[i];
    S.n += 3;
    if (D[i] <= 8 && bits(out[cnt + i]) != bits(got)) S.fail("D %d x %.17g: es_poly_eval %a, es_poly_eval_r<8> %a", D[i], x[i], got, out[cnt + i]);
    if (bits(out[2 * cnt + i]) != bits(got)) S.fail("D %d x %.17g: es_poly_eval %a, es_poly_eval_r<12> %a", D[i], x[i], got, out[2 * cnt + i]);
    const ld bound = powl(1 + U53, 3 * D[i] + 4) - 1;
    if (ref == 0) { if (got != 0) S.fail("D %d x %.17g: %a, reference 0", D[i], x[i], got); continue; }
    const ld err = fabsl((ld)got - ref) / ref;
    if (err > worst[D[i]]) worst[D[i]] = err;
    S.err(err / bound);
    if (!(err <= bound)) S.fail("D %d x %.17g: es_poly_eval %a, reference %.21Lg (%.2Lf x 2^-53 > %d)", D[i], x[i], got, ref, err / U53, 3 * D[i] + 4);
  }
  for (int d : Ds) printf("  D %2d: max relative error %.2Lf x 2^-53 (bound %d)\n", d, worst[d] / U53, 3 * d + 4);
  return S.done();
}

// ---------------------------------------------------------------------------------------------------------- brent
// objectives from fma, +, x and / only: the same bits on host and device without contraction
struct BrObj {
  int kind;
  double p[4];
  double tol;
  int itmax;
};
__host__ __device__ inline double br_f(const BrObj& o, double x) {
  switch (o.kind) {
    case 0: { const double t = x - o.p[0], t2 = t * t; return fma(o.p[1], t2 * t2, fma(o.p[2], t2, o.p[3])); }   // convex quartic
    case 1: return fma(o.p[0], x, o.p[1] * (x * x * x)) + o.p[2];                                              // increasing
    case 2: return o.p[2] - fma(o.p[0], x, o.p[1] * (x * x * x));                                              // decreasing
    case 3: return o.p[0];                                                                                       // constant
    case 4: { const double s = x - o.p[0], t = x - o.p[1]; return fma(o.p[2], (s * s) * (t * t), o.p[3] * x); } // two minima
    case 5: { const double t = x - o.p[0]; return o.p[2] - o.p[1] / fma(t, t, o.p[1]); }                         // sharp, near 0.0001
    default: return fma(x + o.p[1], x, o.p[0]) / fma(fma(o.p[3], x, o.p[2]), x, 1.0);                            // rational
  }
}
__global__ void k_brent_sm(const BrObj* o, int cnt, double* mn, double* fmin, int* nev, int* ok) {
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    const BrObj ob = o[i];
    PmBrent B;
    pm_brent_init(B, ob.tol, ob.itmax);
    while (pm_brent_feed(B, br_f(ob, B.x))) {}
    mn[i] = B.mn; fmin[i] = B.fmin; nev[i] = B.nev; ok[i] = B.ok;
  }
}

// OptimizeFrequency + ScalarMinimizer::Brent in the loop form of the oracle's optimize() (restated, not linked): three
// counted evaluations (only f(b) is read), b = 0.9999 the starting minimum
static double h_sign(double a, double b) { return b >= 0 ? fabs(a) : -fabs(a); }
static bool host_brent(const BrObj& o, double& omin, double& ofmin, int& nev) {
  double a = 0.0001, b = 0.9999, cc = 0.5;
  const double fb = br_f(o, b);
  nev = 3;
  const double tol = o.tol;
  double min = b, fmin = fb, w = b, v = b, fw = fb, fv = fb, delta = 0.0, u, fu, d = 0.0, temp;
  for (int iter = 1; iter <= o.itmax; iter++) {
    const double middle = 0.5 * (a + cc);
    const double tol1 = tol * fabs(min) + 3.0e-10;
    const double tol2 = 2.0 * tol1;
    if (fabs(min - middle) <= (tol2 - 0.5 * (cc - a))) { omin = min; ofmin = fmin; return true; }
    if (fabs(delta) > tol1) {
      double r = (min - w) * (fmin - fv);
      double q = (min - v) * (fmin - fw);
      double p = (min - v) * q - (min - w) * r;
      q = 2.0 * (q - r);
      if (q > 0.0) p = -p;
      q = fabs(q);
      temp = delta; delta = d;
      if (fabs(p) >= fabs(0.5 * q * temp) || p <= q * (a - min) || p >= q * (cc - min)) {
        delta = min >= middle ? a - min : cc - min;
        d = 0.38196601 * delta;
      } else {
        d = p / q;
        u = min + d;
        if (u - a < tol2 || cc - u < tol2) d = h_sign(tol1, middle - min);
      }
    } else {
      delta = min >= middle ? a - min : cc - min;
      d = 0.38196601 * delta;
    }
    u = fabs(d) >= tol1 ? min + d : min + h_sign(tol1, d);
    fu = br_f(o, u);
    nev++;
    if (fu <= fmin) {
      if (u >= min) a = min; else cc = min;
      v = w; w = min; min = u;
      fv = fw; fw = fmin; fmin = fu;
    } else {
      if (u < min) a = u; else cc = u;
      if (fu <= fw || w == min) { v = w; w = u; fv = fw; fw = fu; }
      else if (fu <= fv || v == min || v == w) { v = u; fv = fu; }
    }
  }
  omin = min; ofmin = fmin;
  return false;
}

static int sec_brent() {
  Sec S{"brent", ": mn, fmin, nev and ok bit for bit", 0};
  std::mt19937_64 rng(0xB4E7);
  std::vector<BrObj> O;
  for (int kind = 0; kind < 7; kind++)
    for (int s = 0; s < 64; s++) {
      BrObj o{};
      o.kind = kind;
      const double u0 = rand_unit(rng), u1 = rand_unit(rng), u2 = rand_unit(rng), u3 = rand_unit(rng);
      switch (kind) {
        case 0: o.p[0] = 0.001 + 0.997 * u0; o.p[1] = 1e4 * u1; o.p[2] = 1e3 * u2 + 1e-3; o.p[3] = 1e5 * (u3 - 0.5); break;
        case 1: case 2: o.p[0] = 1e3 * u0 + 1e-6; o.p[1] = 1e4 * u1; o.p[2] = 1e5 * (u2 - 0.5); break;
        case 3: o.p[0] = s == 0 ? 0.0 : 1e6 * (u0 - 0.5); break;
        case 4: o.p[0] = 0.05 + 0.3 * u0; o.p[1] = 0.6 + 0.35 * u1; o.p[2] = 1e4 * u2 + 1; o.p[3] = 20 * (u3 - 0.5); break;
        case 5: o.p[0] = 0.0001 + 0.0005 * u0; o.p[1] = 1e-9 + 1e-7 * u1; o.p[2] = 1e3 * u2; break;
        default: o.p[0] = 0.5 + 4 * u0; o.p[1] = -2 * u1; o.p[2] = 3 * u2; o.p[3] = 5 * u3; break;   // denominator >= 1 on (0, 1)
      }
      for (double tol : {1e-4, 1e-8})
        for (int itmax : {200, 5}) { o.tol = tol; o.itmax = itmax; O.push_back(o); }
    }
  const int cnt = (int)O.size();
  Buf<BrObj> dO(O);
  Buf<double> dmn(cnt), dfm(cnt);
  Buf<int> dnev(cnt), dok(cnt);
  k_brent_sm<<<1, 256>>>(dO.p, cnt, dmn.p, dfm.p, dnev.p, dok.p);
  ran();
  const std::vector<double> mn = dmn.get(), fm = dfm.get();
  const std::vector<int> nev = dnev.get(), ok = dok.get();
  int stuck = 0, conv = 0;
  for (int i = 0; i < cnt; i++) {
    double hmin, hfmin;
    int hnev;
    const bool hok = host_brent(O[i], hmin, hfmin, hnev);
    (hok ? conv : stuck)++;
    S.n++;
    if (bits(mn[i]) != bits(hmin) || bits(fm[i]) != bits(hfmin) || nev[i] != hnev || (ok[i] != 0) != hok)
      S.fail("objective %d set %d tol %g itmax %d: device mn %a fmin %a nev %d ok %d, host mn %a fmin %a nev %d ok %d", O[i].kind,
             i / 4 % 64, O[i].tol, O[i].itmax, mn[i], fm[i], nev[i], ok[i], hmin, hfmin, hnev, (int)hok);
  }
  printf("  %d runs converged, %d ended at itmax (host reference)\n", conv, stuck);
  return S.done();
}

// ----------------------------------------------------------------------------------------------------------
int main(int argc, char** argv) {
  struct { const char* name; int (*fn)(); } secs[] = {{"div", sec_div},         {"log", sec_log},   {"wave", sec_wave},    {"block", sec_block},
                                                      {"quartic", sec_quartic}, {"poly", sec_poly}, {"espoly", sec_espoly}, {"brent", sec_brent}};
  int rc = 0, ran_any = 0;
  for (auto& s : secs)
    if (argc < 2 || !strcmp(argv[1], s.name)) { rc |= s.fn(); ran_any = 1; }
  if (!ran_any) { fprintf(stderr, "num_check: no section '%s' (div log wave block quartic poly espoly brent)\n", argv[1]); return 2; }
  return rc;
}
