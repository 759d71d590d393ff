// es_jit.cpp -- see es_jit.h.
#include "es_jit.h"
#include <hip/hiprtc.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include "../../include/polymutt_engine.h"
#include "jit_headers.inc"   // kBrentCoreH, kLogTableH: csrc/brent_core.h and csrc/log_table.h as text

namespace pmjit {
namespace {

constexpr int MALE = 1, FEMALE = 2;

// A homogeneous polynomial in (f, g = 1 - f) of degree d: coefficient names c[a] of f^a g^(d - a) ("" = zero).
struct Poly {
  int d = 0;
  std::vector<std::string> c;
};

std::string lit(double x) {   // exact hexadecimal literal
  char b[64];
  snprintf(b, sizeof b, "%a", x);
  return b;
}

struct Gen {
  std::string code;
  int nv = 0;
  long ops = 0;   // FP64 operations emitted (each mul, add or fma one; table loads not counted)
  std::map<std::string, std::string> memo;   // expression -> value: identical computations share one value
  std::string def(const std::string& expr) {
    auto it = memo.find(expr);
    if (it != memo.end()) return it->second;
    if (expr.compare(0, 3, "lk[") != 0) ops++;
    std::string v = "v" + std::to_string(nv++);
    code += "  const double " + v + " = " + expr + ";\n";
    memo[expr] = v;
    return v;
  }
  // acc + x * y (acc empty: x * y); "1" factors elided
  std::string mac(const std::string& acc, const std::string& x, const std::string& y) {
    const bool x1 = x == "1.0", y1 = y == "1.0";
    const std::string prod = x1 ? y : y1 ? x : "";
    if (acc.empty()) return prod.empty() ? def(x + " * " + y) : prod;
    if (!prod.empty()) return def(acc + " + " + prod);
    return def("fma(" + x + ", " + y + ", " + acc + ")");
  }
  Poly zero(int d) { Poly p; p.d = d; p.c.assign(d + 1, ""); return p; }
  Poly mul(const Poly& A, const Poly& B) {
    Poly R = zero(A.d + B.d);
    for (int a = 0; a <= R.d; a++)
      for (int u = std::max(0, a - B.d); u <= std::min(a, A.d); u++)
        if (!A.c[u].empty() && !B.c[a - u].empty()) R.c[a] = mac(R.c[a], A.c[u], B.c[a - u]);
    return R;
  }
  // sum_t w_t P_t (all of degree d)
  Poly lincomb(const std::vector<std::pair<double, const Poly*>>& terms, int d) {
    Poly R = zero(d);
    for (int a = 0; a <= d; a++)
      for (auto& t : terms) {
        if (t.first == 0.0 || t.second->c[a].empty()) continue;
        R.c[a] = mac(R.c[a], t.first == 1.0 ? std::string("1.0") : lit(t.first), t.second->c[a]);
      }
    return R;
  }
  Poly add(const Poly& A, const Poly& B) {   // same degree
    Poly R = zero(A.d);
    for (int a = 0; a <= A.d; a++) {
      if (A.c[a].empty()) R.c[a] = B.c[a];
      else if (B.c[a].empty()) R.c[a] = A.c[a];
      else R.c[a] = def(A.c[a] + " + " + B.c[a]);
    }
    return R;
  }
};

// transmission_BA of the class for an offspring of sex csex (GetTransmissionProb_BA :1059-1075)
double tba(const double (*T)[27], int chrom, int csex, int i, int j, int k) {
  const int o = i * 9 + j * 3 + k;
  if (chrom == PM_CHR_X) return csex == MALE ? T[2][o] : T[1][o];
  if (chrom == PM_CHR_Y) return csex == MALE ? T[3][o] : 1.0;
  if (chrom == PM_CHR_MT) return T[4][o];
  return T[0][o];
}

// the shape key: everything the generated code depends on
std::string shape_key(const Family& F) {
  std::string k = std::to_string(F.n) + ":" + std::to_string(F.nf) + ":";
  for (int i = 0; i < F.n; i++) {
    k += F.founder[i] ? 'F' : 'o';
    k += (char)('0' + F.sex[i]);   // (child sex of the X/Y transmission, chrY females)
  }
  for (auto& s : F.steps) k += ":" + std::to_string(s.x) + "," + std::to_string(s.y);
  return k;
}

// One family shape's hoisting as a device function: the polynomial of FamilyLikelihoodES' BA peel in (f, g).
// fused: the ep_brent_jit form -- inlined, the D + 1 coefficients into the caller's register array out[0..D] (no degree
// word); *deg = D.
std::string gen_family(const Family& F, int chrom, const double (*T)[27], const std::string& name, double* ops,
                       bool fused = false, int* deg = nullptr) {
  Gen G;
  const int n = F.n;
  const bool X = chrom == PM_CHR_X, Y = chrom == PM_CHR_Y, MT = chrom == PM_CHR_MT;
  std::map<std::pair<int, int>, std::string> pen;   // (person, state) -> loaded likelihood
  auto penv = [&](int i, int j) {
    auto key = std::make_pair(i, j);
    auto it = pen.find(key);
    if (it != pen.end()) return it->second;
    static const char* plane[3] = {"P11", "P12", "P22"};
    std::string v = G.def(std::string("lk[") + plane[j] + "[p0 + " + std::to_string(i) + "]]");
    pen[key] = v;
    return v;
  };
  // InitializePartials_BA x SetFounderPriors_BA (:1449-1465, :666-687)
  std::vector<std::vector<Poly>> P(n, std::vector<Poly>(3));
  for (int i = 0; i < n; i++) {
    const int sx = F.sex[i];
    const bool fo = F.founder[i] && i < F.nf;
    const bool yf = Y && sx == FEMALE;
    const int d = !fo ? 0 : yf ? 0 : (((X || Y) && sx == MALE) || MT) ? 1 : 2;
    for (int j = 0; j < 3; j++) {
      Poly p = G.zero(d);
      if (yf) p.c[0] = "1.0";
      else if (!fo) p.c[0] = penv(i, j);
      else if (d == 2) p.c[2 - j] = j == 1 ? G.def("2.0 * " + penv(i, j)) : penv(i, j);   // f^2, 2fg, g^2
      else if (j != 1) p.c[j == 0 ? 1 : 0] = penv(i, j);                                    // f, 0, g
      P[i][j] = p;
    }
  }
  std::map<int, std::vector<Poly>> M;   // marriage partials by slot: [i * 3 + j]
  int fin = -1;
  for (const int2& S : F.steps) {
    const int type = S.x & 255, from0 = (S.x >> 8) & 255, from1 = (S.x >> 16) & 255, to0 = (S.x >> 24) & 255;
    const int slot = (S.y >> 8) & 255, create = (S.y >> 16) & 1, fa2mo = (S.y >> 17) & 1;
    fin = to0;
    if (type == 1) {   // peelOffspring2Parents_BA (:1105-1130): M(i, j) *= sum_k T(i, j, k) P_off[k]
      const int off = from0, csex = F.sex[off], da = P[off][0].d;
      std::vector<Poly> Sij(9);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          std::vector<std::pair<double, const Poly*>> t;
          for (int k = 0; k < 3; k++) t.push_back({tba(T, chrom, csex, i, j, k), &P[off][k]});
          Sij[i * 3 + j] = G.lincomb(t, da);
        }
      if (create || !M.count(slot)) M[slot] = Sij;
      else
        for (int e = 0; e < 9; e++) M[slot][e] = G.mul(M[slot][e], Sij[e]);
    } else if (type == 2) {   // peelSpouse2Spouse_BA (:1182-1230): P_to[i] *= sum_j P_from[j] M(j, i)
      const int sf = from0, stt = to0;
      for (int i = 0; i < 3; i++) {
        Poly sum;
        bool first = true;
        for (int j = 0; j < 3; j++) {
          Poly term = slot == 255 ? P[sf][j] : G.mul(P[sf][j], M[slot][fa2mo ? j * 3 + i : i * 3 + j]);
          sum = first ? term : G.add(sum, term);
          first = false;
        }
        P[stt][i] = G.mul(P[stt][i], sum);
      }
    } else {   // peelParents2Offspring_BA (:1260-1286): P_off[k] *= sum_ij P_fa[i] M(i, j) P_mo[j] T(i, j, k)
      const int fa = from0, mo = from1, off = to0, csex = F.sex[off];
      std::vector<Poly> W(9);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          const Poly fm = slot == 255 ? P[fa][i] : G.mul(P[fa][i], M[slot][i * 3 + j]);
          W[i * 3 + j] = G.mul(fm, P[mo][j]);
        }
      for (int k = 0; k < 3; k++) {
        std::vector<std::pair<double, const Poly*>> t;
        for (int e = 0; e < 9; e++) t.push_back({tba(T, chrom, csex, e / 3, e % 3, k), &W[e]});
        const Poly Sk = G.lincomb(t, W[0].d);
        P[off][k] = G.mul(P[off][k], Sk);
      }
    }
  }
  // CalculateLikelihood_BA (:1013-1032): the final person's partials summed
  Poly L = G.add(G.add(P[fin][0], P[fin][1]), P[fin][2]);
  if (deg) *deg = L.d;
  *ops = (double)G.ops;
  if (fused) {
    std::string out = "__device__ __forceinline__ void " + name +
                      "(const unsigned char* __restrict__ P11, const unsigned char* __restrict__ P12, "
                      "const unsigned char* __restrict__ P22, int p0, const double* __restrict__ lk, double* out) {\n" + G.code;
    for (int a = 0; a <= L.d; a++) out += "  out[" + std::to_string(a) + "] = " + (L.c[a].empty() ? "0.0" : L.c[a]) + ";\n";
    return out + "}\n";
  }
  std::string out = "__device__ __attribute__((noinline)) void " + name +
                    "(const unsigned char* __restrict__ P11, const unsigned char* __restrict__ P12, "
                    "const unsigned char* __restrict__ P22, int p0, const double* __restrict__ lk, double* __restrict__ out, "
                    "int os, int dcap) {\n" + G.code;
  for (int a = 0; a <= L.d; a++) out += "  out[" + std::to_string(a) + " * os] = " + (L.c[a].empty() ? "0.0" : L.c[a]) + ";\n";
  out += "  out[(dcap - 1) * os] = " + std::to_string(L.d) + ".0;\n}\n";
  return out;
}

const char* kPrologue = R"(
typedef unsigned char uint8_t;
struct Args {
  const int* items; const int* counts; const uint8_t* ref; const int* res; const uint8_t* pl; const double* lktab;
  double* coef; const int* slot_e; const int* slot_sig; const int* slot_p0;
  const double* T10; const double* T10dn; const double* tba; unsigned long long* prof; const int* pair_k;
  int list, it0, it1, nslots, np, T, max_ext, dcap, vcf, res_words, res_a1, res_a2, denovo, group, npairs;
};
__device__ __forceinline__ int gi(int b1, int b2) {
  return b1 < b2 ? (b1 - 1) * (10 - b1) / 2 + (b2 - b1) : (b2 - 1) * (10 - b2) / 2 + (b1 - b2);
}
__device__ __forceinline__ void cfg_alleles(int cfg, int r, int* a1, int* a2) {   // main.cpp:458-529, PedigreeGLF.h:14-53
  const int ts = r == 1 ? 3 : r == 2 ? 4 : r == 3 ? 1 : 2, tv1 = (r == 1 || r == 3) ? 2 : 1, tv2 = (r == 1 || r == 3) ? 4 : 3;
  switch (cfg) {
    case 0: *a1 = r; *a2 = (r == 4) ? 3 : r + 1; break;
    case 1: *a1 = r; *a2 = ts; break;
    case 2: *a1 = r; *a2 = tv1; break;
    case 3: *a1 = r; *a2 = tv2; break;
    case 4: *a1 = ts; *a2 = tv1; break;
    case 5: *a1 = ts; *a2 = tv2; break;
    default: *a1 = tv1; *a2 = tv2; break;
  }
}
)";

std::string gen_kernel(const std::vector<std::string>& shapes) {
  std::string s = R"(
extern "C" __global__ void __launch_bounds__(256) es_hoist_jit(Args A) {
  __shared__ double lk[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) lk[i] = A.lktab[i];
  __syncthreads();
  const int nItems = min(A.counts[A.list], A.it1);
  if (nItems <= A.it0) return;
  const long long units = (long long)(nItems - A.it0) * A.nslots;
  for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (long long)gridDim.x * blockDim.x) {
    const int uq = (int)(u / A.nslots), k = (int)(u - (long long)uq * A.nslots);
    const int it = A.it0 + uq;
    const int item = A.items[it];
    const int site = item >> 3, cfg = item & 7, r = A.ref[site];
    int a1, a2;
    if (A.vcf) { a1 = r & 15; a2 = r >> 4; }
    else if (cfg == 7) { a1 = A.res[(size_t)site * A.res_words + A.res_a1]; a2 = A.res[(size_t)site * A.res_words + A.res_a2]; }
    else cfg_alleles(cfg, r, &a1, &a2);
    const uint8_t* pl = A.pl + (size_t)site * A.np * 10;
    const uint8_t* P11 = pl + (size_t)gi(a1, a1) * A.np;
    const uint8_t* P12 = pl + (size_t)gi(a1, a2) * A.np;
    const uint8_t* P22 = pl + (size_t)gi(a2, a2) * A.np;
    const int e = A.slot_e[k], q = e / A.T;
    double* out = A.coef + ((size_t)uq * A.max_ext + q) * A.dcap * A.T + (e - q * A.T);
    switch (A.slot_sig[k]) {
)";
  for (size_t i = 0; i < shapes.size(); i++)
    s += "      case " + std::to_string(i) + ": " + shapes[i] + "(P11, P12, P22, A.slot_p0[k], lk, out, A.T, A.dcap); break;\n";
  s += "    }\n  }\n}\n";
  return s;
}


// ---------------------------------------------------------------------------------------------------------------
// Genotype posteriors of one family shape (CalcPostProb_SingleExtendedPed_BA, FamilyLikelihoodSeq.cpp:171-216): for
// every person j and genotype s, the reference-order numeric BA peel at freq with j's penetrances zeroed but for s
// (FillZeroPenetrance :327-356).  The operations and their order are d_es_lk<3>'s (engine.hip), hence the
// reference's, term by term; folding x * 1 -> x, dropping + 0 and 0-products (every value is finite and >= 0) keeps
// every bit.  Computations that do not depend on j's zeroed penetrance are generated once (Gen::def memo), so the 3n
// peels of a family share their common prefix.
struct NumPeel {
  Gen& G;
  explicit NumPeel(Gen& g) : G(g) {}
  static bool is0(const std::string& x) { return x == "0.0"; }
  std::string mul(const std::string& x, const std::string& y) {
    if (is0(x) || is0(y)) return "0.0";
    if (x == "1.0") return y;
    if (y == "1.0") return x;
    return G.def(x + " * " + y);
  }
  std::string add(const std::string& acc, const std::string& x) {   // acc + x, acc "" = the sum's 0.0 start
    if (acc.empty()) return x;
    if (is0(x)) return acc;
    if (is0(acc)) return x;
    return G.def(acc + " + " + x);
  }
};

std::string gen_post_family(const Family& F, int chrom, const double (*T)[27], const std::string& name) {
  Gen G;
  NumPeel N(G);
  const int n = F.n;
  const bool X = chrom == PM_CHR_X, Y = chrom == PM_CHR_Y, MT = chrom == PM_CHR_MT;
  static const char* plane[3] = {"P11", "P12", "P22"};
  std::string body;
  // founder priors (d_es_lk: pr[] per founder, same expressions)
  const std::string q0 = G.def("fq * fq"), q1 = G.def("2 * fq * (1 - fq)"), q2 = G.def("(1 - fq) * (1 - fq)");
  const std::string h0 = "fq", h2 = G.def("1 - fq");
  std::vector<std::vector<std::string>> pen(n, std::vector<std::string>(3));
  for (int i = 0; i < n; i++)
    for (int s = 0; s < 3; s++) pen[i][s] = G.def(std::string("lk[") + plane[s] + "[p0 + " + std::to_string(i) + "]]");
  auto peel = [&](int zp, int zs) {
    std::vector<std::vector<std::string>> P(n, std::vector<std::string>(3));
    for (int i = 0; i < n; i++) {
      const int sx = F.sex[i];
      const bool fo = F.founder[i] != 0;
      std::string pr[3] = {"0.0", "0.0", "0.0"};
      if (i < F.nf) {
        pr[0] = q0; pr[1] = q1; pr[2] = q2;
        if (X && sx == MALE) { pr[0] = h0; pr[1] = "0.0"; pr[2] = h2; }
        if (Y) { if (sx == MALE) { pr[0] = h0; pr[1] = "0.0"; pr[2] = h2; } else { pr[0] = pr[1] = pr[2] = "1.0"; } }
        if (MT) { pr[0] = h0; pr[1] = "0.0"; pr[2] = h2; }
      }
      for (int s = 0; s < 3; s++) {
        const std::string pe = (zp == i && s != zs) ? std::string("0.0") : pen[i][s];
        P[i][s] = (Y && sx == FEMALE) ? std::string("1.0") : (fo ? N.mul(pr[s], pe) : pe);
      }
    }
    std::map<int, std::vector<std::string>> M;
    int fin = -1;
    for (const int2& S : F.steps) {
      const int type = S.x & 255, from0 = (S.x >> 8) & 255, from1 = (S.x >> 16) & 255, to0 = (S.x >> 24) & 255;
      const int slot = (S.y >> 8) & 255, create = (S.y >> 16) & 1, fa2mo = (S.y >> 17) & 1;
      fin = to0;
      if (type == 1) {
        const int off = from0, csex = F.sex[off];
        if (create || !M.count(slot)) M[slot].assign(9, "1.0");
        for (int i = 0; i < 3; i++)
          for (int j = 0; j < 3; j++) {
            std::string sum;
            for (int k = 0; k < 3; k++) {
              const double t = tba(T, chrom, csex, i, j, k);
              sum = N.add(sum, t == 0.0 ? std::string("0.0") : N.mul(t == 1.0 ? std::string("1.0") : lit(t), P[off][k]));
            }
            M[slot][i * 3 + j] = N.mul(M[slot][i * 3 + j], sum.empty() ? std::string("0.0") : sum);
          }
      } else if (type == 2) {
        const int sf = from0, stt = to0;
        for (int i = 0; i < 3; i++) {
          std::string sum;
          for (int j = 0; j < 3; j++) {
            if (slot == 255) sum = N.add(sum, P[sf][j]);
            else sum = N.add(sum, N.mul(P[sf][j], M[slot][fa2mo ? j * 3 + i : i * 3 + j]));
          }
          P[stt][i] = N.mul(P[stt][i], sum.empty() ? std::string("0.0") : sum);
        }
      } else {
        const int fa = from0, mo = from1, off = to0, csex = F.sex[off];
        std::string sum[3];
        for (int i = 0; i < 3; i++)
          for (int j = 0; j < 3; j++) {
            const std::string w = slot == 255 ? N.mul(P[fa][i], P[mo][j]) : N.mul(N.mul(P[fa][i], M[slot][i * 3 + j]), P[mo][j]);
            for (int k = 0; k < 3; k++) {
              const double t = tba(T, chrom, csex, i, j, k);
              sum[k] = N.add(sum[k], t == 0.0 ? std::string("0.0") : N.mul(t == 1.0 ? std::string("1.0") : lit(t), w));
            }
          }
        for (int k = 0; k < 3; k++) P[off][k] = N.mul(P[off][k], sum[k].empty() ? std::string("0.0") : sum[k]);
      }
    }
    std::string L;
    for (int i = 0; i < 3; i++) L = N.add(L, P[fin][i]);
    return L.empty() ? std::string("0.0") : L;
  };
  for (int j = 0; j < n; j++) {
    const int sx = F.sex[j];
    if (Y && sx == FEMALE) {   // CalcPostProb_SingleExtendedPed_BA: chrY females get no posterior ('.')
      body += "  emit(calls, out0 + p0 + " + std::to_string(j) + ", 0.0, 0.0, 0.0, " + std::to_string((int)PM_LBL_DOT) +
              ", thr, vcf, 1);\n";
      continue;
    }
    const std::string l0 = peel(j, 0), l1 = peel(j, 1), l2 = peel(j, 2);
    const int lab = (Y || MT || (X && sx == MALE)) ? PM_LBL_VCF_HAPLOID : PM_LBL_VCF_DIPLOID;   // d_vcf_label
    body += "  emit(calls, out0 + p0 + " + std::to_string(j) + ", " + l0 + ", " + l1 + ", " + l2 + ", " + std::to_string(lab) +
            ", thr, vcf, 0);\n";
  }
  return "__device__ __attribute__((noinline)) void " + name +
         "(const unsigned char* __restrict__ P11, const unsigned char* __restrict__ P12, const unsigned char* __restrict__ P22, "
         "int p0, const double* __restrict__ lk, double fq, const double* __restrict__ thr, void* calls, size_t out0, int vcf) {\n" +
         G.code + body + "}\n";
}

const char* kPostPrologue = R"(
struct PostArgs {
  const int* counts; const int* row_site; const char* res; const uint8_t* pl; const double* lktab; const double* gq_thr;
  void* calls; const int* fam_p0; const int* fam_sig;
  int nfams, np, vcf, res_bytes, off_a1, off_a2, off_maxidx, off_af;
  double theta;
};
struct GenoCall { double dosage; short best; short gq; signed char label; signed char pad[3]; };
struct VcfCall { signed char best; signed char gq; signed char label; signed char pad; };
// d_gq (engine.hip): GQ of OutputVCF :1818-1820 from the host's glibc thresholds, exact for every double
__device__ __forceinline__ int gq_of(double pb, const double* thr) {
  const double q = 1. - pb;
  const int g = (int)(-3.01029995664f * __builtin_amdgcn_logf((float)q) + 0.5f);   // (bare v_log_f32: see d_gq)
  const int base = min(max(g - 2, 0), 96);
  int k = base;
  for (int i = 0; i < 4; i++) k += q < thr[base + i] ? 1 : 0;
  return pb > 0.9999999999 ? 100 : k;
}
// k_posterior_es's tail: post = l / sum, best = d_best3(l), GQ of post[best], DS = post12 + 2 post22
__device__ __forceinline__ void emit(void* calls, size_t idx, double l11, double l12, double l22, int label, const double* thr,
                                     int vcf, int zero) {
  double post[3] = {0.0, 0.0, 0.0};
  int best = 0;
  if (!zero) {
    const double sum = l11 + l12 + l22;
    if (sum != 0) { post[0] = l11 / sum; post[1] = l12 / sum; post[2] = l22 / sum; }
    double m = l11;
    if (l12 > m) { m = l12; best = 1; }
    if (l22 > m) { m = l22; best = 2; }
  }
  const int gq = gq_of(post[best], thr);
  if (vcf) {
    VcfCall c; c.best = (signed char)best; c.gq = (signed char)gq; c.label = (signed char)label; c.pad = 0;
    ((VcfCall*)calls)[idx] = c;
    return;
  }
  GenoCall c; c.dosage = post[1] + post[2] * 2; c.best = (short)best; c.gq = (short)gq; c.label = (signed char)label;
  c.pad[0] = c.pad[1] = c.pad[2] = 0;
  ((GenoCall*)calls)[idx] = c;
}
)";

std::string gen_post_kernel(const std::vector<std::string>& shapes) {
  std::string s = R"(
extern "C" __global__ void __launch_bounds__(256) es_post_jit(PostArgs A) {
  __shared__ double lk[256];
  __shared__ double thr[101];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) lk[i] = A.lktab[i];
  for (int i = threadIdx.x; i < 101; i += blockDim.x) thr[i] = A.gq_thr[i];
  __syncthreads();
  const long long work = (long long)A.counts[3] * A.nfams;
  for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < work; u += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(u / A.nfams), k = (int)(u - (long long)row * A.nfams);
    const int site = A.row_site[row];
    const char* R = A.res + (size_t)site * A.res_bytes;
    const int a1 = *(const int*)(R + A.off_a1), a2 = *(const int*)(R + A.off_a2);
    const double fq = (*(const int*)(R + A.off_maxidx) == 0) ? 1 - A.theta : *(const double*)(R + A.off_af);   // main.cpp:576-587
    const uint8_t* pl = A.pl + (size_t)site * A.np * 10;
    const uint8_t* P11 = pl + (size_t)gi(a1, a1) * A.np;
    const uint8_t* P12 = pl + (size_t)gi(a1, a2) * A.np;
    const uint8_t* P22 = pl + (size_t)gi(a2, a2) * A.np;
    const size_t out0 = (size_t)row * A.np;
    switch (A.fam_sig[k]) {
)";
  for (size_t i = 0; i < shapes.size(); i++)
    s += "      case " + std::to_string(i) + ": " + shapes[i] + "(P11, P12, P22, A.fam_p0[k], lk, fq, thr, A.calls, out0, A.vcf); break;\n";
  s += "    }\n  }\n}\n";
  return s;
}


// ---------------------------------------------------------------------------------------------------------------
// Wave-cooperative hoisting (--denovo engines: 10-state peels, whose marriage partials -- 100 entries x coefficients
// -- do not fit one thread's registers).  One (item, family) per half-wave, as engine.hip's generic k_es_hoist per
// wave, but compiled per family shape: the workspace layout, every step's degrees and every loop bound are constants,
// so a phase is a few unrolled multiply-adds per lane between wave-level barriers, with no schedule or layout loads
// and no run-time divisions.  Variants per shape: 10-state (de novo items), bi-allelic (cfg-7 items), and "top"
// (the de novo monomorphism item: the f^D coefficient only, every degree 0).
//
// The one configuration (the measured-and-rejected alternatives are in the history):
//  * family pairs: each half-wave (kWl = 32 lanes) hoists one of two same-shape families of the task in its own
//    workspace slice, so every phase whose elements fit 32 lanes (type-2 steps over 10 states, founder-sparse type-1
//    runs over 30 pairs, the final sum) does two families' work per instruction;
//  * partials are read across lanes through LDS only;
//  * a founder read only by pristine type-2 steps is never stored: its terms read the penetrance from PEN;
//  * a person first used as the to-person of a type-2 step has its initial partial formed in that step's lanes;
//  * independent type-2 steps of one shape share a phase, 16 lanes each;
//  * the per-item rest's regions are packed by live range.
constexpr int kFpw = 2;          // families per wave
constexpr int kWl = 64 / kFpw;   // lanes per family

// The generator's switches: generate() fills them from the environment and passes them down
struct Opts {
  bool prof = false;     // PM_ES_PROF=1: es_hoist_wave accumulates per-part clock cycles into Args::prof
  bool sp3 = true;       // PM_ES_SP3=0: type-3 steps with a founder parent over all 100 pairs
  bool t3z = true;       // PM_ES_T3Z=0: dense type-3 child sums over all 100 parent pairs of the global table
  bool layout = false;   // PM_JIT_LAYOUT: workspace layouts and static lane occupancy to stderr
  bool steps = false;    // PM_JIT_STEPS: every step's operations to stderr
};

std::string S(long v) { return std::to_string(v); }

struct StepDeg { int a, b, c, e; };
// the founder-sparse rows of a type-1 run (sparse_of): the founder's non-zero states, its side of the pair, compact rows
struct Sparse { std::vector<std::pair<int, int>> terms; bool father = false, compact = false; };

// What the generated function of one (family shape, variant, part) depends on: degrees, classifications and the
// workspace layout.  analyse_wave_family() fills it; the emit_* functions below only read it.
// part (10-state variants only): 0 the whole peel; 1 the cfg-independent prefix -- the 10-state penetrances of
// non-founders no step changes and the type-1 steps that peel them into marriage partials no cfg-dependent step
// writes (leaf steps, run first: nothing they read or write is touched by an earlier step) -- and 2 the rest (the
// other persons' partials, the other steps, the final sum).  Part 1 once and part 2 per item give part 0's values for
// the de novo items of one site (they differ only in the founder priors' genotypes; the top variant's leaf steps are
// the same degree-0 products).  Parts lay out the workspace by the 10-state variant's degrees, top or not.
struct WaveFamily {
  const Family& F;
  int chrom, NS;
  bool top;
  int part;
  std::string name;
  int n, nst;
  std::vector<int> d0, dP, capP;   // persons: initial and final degree, capacity (coefficients per state)
  std::map<int, int> capM;         // marriage slots: capacity
  int tmp = 1;                     // the type-3 products W(i, j)
  std::vector<StepDeg> sd;         // the steps' operand degrees
  // leaf steps (part 1) and the persons only they read; pristine[k]: the founder "from" of type-2 step k still holds
  // its prior x penetrance partial (3 non-zero states), so the step sums over those 3 states only; sp3[k]: a
  // founder-sparse type-3 step
  std::vector<char> leaf, leafp, pristine, sp3;
  // persons without a workspace region: penf, founders read only through pristine type-2 steps (the terms read PEN);
  // penp, leaf offspring (the leaf steps read PEN); iinit, persons whose initial partial their type-2 step forms
  std::vector<char> penf, penp, iinit;
  std::map<int, int> crows;        // compactly stored marriage partials: slot -> rows
  std::map<int, int> leafs;        // the marriage slots the leaf steps write
  std::vector<int> po;             // offsets: persons
  std::map<int, int> mo;           // marriage slots
  int LSZ = 0, NSZ = 0, TB = 0;    // the leaf prefix's doubles, the rest's, the type-3 products' offset
  int ws = 0;                      // workspace doubles

  int type(int k) const { return F.steps[k].x & 255; }
  int from0(int k) const { return (F.steps[k].x >> 8) & 255; }
  int from1(int k) const { return (F.steps[k].x >> 16) & 255; }
  int to0(int k) const { return (F.steps[k].x >> 24) & 255; }
  int slot(int k) const { return (F.steps[k].y >> 8) & 255; }
  bool create(int k) const { return (F.steps[k].y >> 16) & 1; }
  bool fa2mo(int k) const { return (F.steps[k].y >> 17) & 1; }
  bool founder(int i) const { return F.founder[i] && i < F.nf; }
  int fdeg(int i) const {   // a founder's prior degree (SetFounderPriors)
    const bool X = chrom == PM_CHR_X, Y = chrom == PM_CHR_Y, MT = chrom == PM_CHR_MT;
    return (Y && F.sex[i] == FEMALE) ? 0 : (((X || Y) && F.sex[i] == MALE) || MT) ? 1 : 2;
  }
  bool inpart(int k) const { return !((part == 1 && !leaf[k]) || (part == 2 && leaf[k])); }
  int mcap(int s) const { auto it = capM.find(s); return it == capM.end() ? 0 : it->second; }
  int mrows(int s) const { auto it = crows.find(s); return it == crows.end() ? NS * NS : it->second; }
  std::string PO(int i) const { return S(po[i]); }
  std::string MO(int s) const { auto it = mo.find(s); return S(it == mo.end() ? 0 : it->second); }
  // a pristine founder's non-zero states (q: 0 g11, 1 g12, 2 g22) and their coefficient u, in the dense loop's order
  // of u at one j: prior x penetrance (SetFounderPriors), the top variant's f^D term only
  std::vector<std::pair<int, int>> pterms(int f) const {
    if (top) return fdeg(f) > 0 ? std::vector<std::pair<int, int>>{{0, 0}} : std::vector<std::pair<int, int>>{{2, 0}, {1, 0}, {0, 0}};
    if (d0[f] == 2) return {{2, 0}, {1, 1}, {0, 2}};
    if (d0[f] == 1) return {{2, 0}, {0, 1}};
    return {{2, 0}, {1, 0}, {0, 0}};
  }
  // runs of consecutive type-1 steps of this part (one phase each in the 10-state code), and their founder-sparse
  // rows: when a run writes one marriage partial and its only later reader is a pristine type-2 step (the founder
  // spouse F peeled into the other), that step reads the rows of F's non-zero states only (2-3 of 10; 1 in the top
  // variant), so only those pairs are computed (lanes over F's states x the spouse's).  In part 2 a partial whose
  // writers all sit in such a run is stored compactly, row q * 10 + spouse state for F's q-th term.
  std::vector<int> run_of(int k0) const {
    std::vector<int> run;
    for (int k2 = k0; k2 < nst; k2++) {
      if (!inpart(k2)) continue;
      if (type(k2) != 1) break;
      run.push_back(k2);
    }
    return run;
  }
  Sparse sparse_of(const std::vector<int>& run) const {
    Sparse sp;
    if (NS != 10 || part == 1 || run.empty()) return sp;
    const int sl0 = slot(run[0]);
    for (int k2 : run)
      if (slot(k2) != sl0) return sp;
    int readers = 0, rk = -1;
    bool writes_after = false, writes_before = false;
    for (int k2 = run.back() + 1; k2 < nst; k2++) {
      if (!inpart(k2) || slot(k2) != sl0) continue;
      if (type(k2) == 1) writes_after = true;
      else { readers++; rk = k2; }
    }
    for (int k2 = 0; k2 < run[0]; k2++)
      if (type(k2) == 1 && slot(k2) == sl0) writes_before = true;
    if (readers == 1 && !writes_after && type(rk) == 2 && pristine[rk]) {
      sp.terms = pterms(from0(rk));
      sp.father = fa2mo(rk);
      sp.compact = part == 2 && !writes_before;
    }
    return sp;
  }
};

// leaf and pristine steps, the compact marriage partials, and the persons that need no workspace region
void classify_steps(WaveFamily& A) {
  const int n = A.n, nst = A.nst, NS = A.NS, part = A.part;
  A.leaf.assign(nst, 0); A.leafp.assign(n, 0); A.pristine.assign(nst, 0);
  A.penf.assign(n, 0); A.penp.assign(n, 0); A.iinit.assign(n, 0);
  if (NS != 10) return;
  std::vector<char> isto(n, 0), touched(n, 0);
  for (int k = 0; k < nst; k++)
    if (A.type(k) != 1) isto[A.to0(k)] = 1;
  for (int k = 0; k < nst; k++) {
    if (A.type(k) == 2 && A.founder(A.from0(k)) && !touched[A.from0(k)]) A.pristine[k] = 1;
    if (A.type(k) != 1) touched[A.to0(k)] = 1;
    // a leaf step reads a non-founder's penetrance partial that no step ever changes
    if (A.type(k) == 1 && !A.founder(A.from0(k)) && !isto[A.from0(k)]) A.leaf[k] = 1;
  }
  // ... into a marriage partial that only leaf steps write, and that no step reads before the last of them
  for (bool changed = true; changed;) {
    changed = false;
    std::map<int, int> nonleaf_writer;
    for (int k = 0; k < nst; k++)
      if (A.type(k) == 1 && !A.leaf[k]) nonleaf_writer[A.slot(k)] = 1;
    for (int k = 0; k < nst; k++) {
      if (A.leaf[k] && nonleaf_writer.count(A.slot(k))) { A.leaf[k] = 0; changed = true; }
      if (A.type(k) == 1 || A.slot(k) == 255) continue;
      for (int k2 = k + 1; k2 < nst; k2++)
        if (A.leaf[k2] && A.type(k2) == 1 && A.slot(k2) == A.slot(k)) { A.leaf[k2] = 0; changed = true; }
    }
  }
  for (int k = 0; k < nst; k++)
    if (A.leaf[k]) {
      A.leafp[A.from0(k)] = 1;
      A.leafs[A.slot(k)] = 1;
    }
  if (part == 2)
    for (int k = 0; k < nst; k++) {
      if (!A.inpart(k) || A.type(k) != 1 || (k > 0 && A.inpart(k - 1) && A.type(k - 1) == 1)) continue;
      const Sparse sp = A.sparse_of(A.run_of(k));
      if (sp.compact) A.crows[A.slot(k)] = 10 * (int)sp.terms.size();
    }
  if (part == 2) {
    const int finp = A.to0(nst - 1);
    for (int i = 0; i < n; i++) A.penf[i] = A.founder(i) && !A.leafp[i] && i != finp;
    for (int k = 0; k < nst; k++) {
      if (!A.inpart(k)) continue;
      const int f0 = A.from0(k), f1 = A.from1(k), t0 = A.to0(k);
      if (A.type(k) == 2) { A.penf[t0] = 0; if (!A.pristine[k]) A.penf[f0] = 0; }
      else if (A.type(k) == 3) A.penf[f0] = A.penf[f1] = A.penf[t0] = 0;
      else A.penf[f0] = 0;
    }
    // persons whose first use is as the to-person of a type-2 step: their initial partial (penetrance, or prior x
    // penetrance) is formed inside that step's lanes instead of being stored and read back
    std::vector<char> seen(n, 0);
    for (int k = 0; k < nst; k++) {
      if (!A.inpart(k)) continue;
      const int f0 = A.from0(k), f1 = A.from1(k), t0 = A.to0(k);
      if (A.type(k) == 2 && !seen[t0] && !A.penf[t0]) A.iinit[t0] = 1;
      seen[f0] = 1;
      if (A.type(k) != 1) seen[t0] = 1;
      if (A.type(k) == 3) seen[f1] = 1;
    }
    for (int i = 0; i < n; i++)
      if (A.leafp[i]) A.iinit[i] = 0;
  }
  // leaf offspring (parts): a non-founder whose partial is its penetrance, never changed, read by leaf steps only --
  // the steps read PEN directly (the site's penetrances stay in the slice for the task), no region, no init
  if (part)
    for (int i = 0; i < n; i++) A.penp[i] = A.leafp[i] && !A.founder(i);
}

// workspace layout: persons' partials, marriage partials, the type-3 products.  Parts put the leaf prefix's regions
// first (a task's items share them)
void layout_workspace(WaveFamily& A) {
  const int n = A.n, nst = A.nst, NS = A.NS, part = A.part, tmp = A.tmp;
  A.po.assign(n, 0);
  int off = 0, LSZ = 0;
  for (int L = part ? 1 : 0; L >= 0; L--) {
    for (int i = 0; i < n; i++)
      if (!part || A.leafp[i] == L) {
        A.po[i] = off;
        if (!A.penf[i] && !A.penp[i]) off += NS * A.capP[i];   // (a PEN-read person: no region)
      }
    for (auto& m : A.capM)
      if (!part || (int)A.leafs.count(m.first) == L) {
        A.mo[m.first] = off;
        off += A.mrows(m.first) * m.second;
      }
    if (L == 1) LSZ = off;
  }
  A.LSZ = LSZ; A.TB = off; A.NSZ = off + tmp - LSZ;
  // Part 2 (the per-item rest, the top rest): its own regions packed by live range.  A region is live from the phase
  // of its first write to the phase of its last read; phases are counted conservatively (consecutive steps of one type
  // share one, a type-3 step is one, the initial partials' phase is -1, the final sum the last), and a region may take
  // the place of one whose live range ended in an earlier phase: a wave_sync lies between them.  Smaller slices ->
  // more slices in a CU's LDS -> more waves in flight.
  if (part == 2 && NS == 10) {
    std::vector<int> ph(nst, -2);
    int cur = -1, prevt = -1;
    for (int k = 0; k < nst; k++) {
      if (!A.inpart(k)) continue;
      const int t = A.type(k);
      if (t != prevt || t == 3) cur++;
      prevt = t;
      ph[k] = cur;
    }
    struct Reg { int size = 0, lo = 1 << 30, hi = -3, off = 0; };
    std::map<int, Reg> rg;   // person i, marriage slot (1000 + slot), the type-3 temporaries (-1)
    auto touch = [&](int id, int size, int p) {
      Reg& r = rg[id];
      r.size = size;
      r.lo = std::min(r.lo, p);
      r.hi = std::max(r.hi, p);
    };
    auto stored = [&](int i) { return !A.leafp[i] && !A.penf[i] && !A.penp[i]; };
    auto msize = [&](int sl) { return A.mrows(sl) * A.mcap(sl); };
    for (int i = 0; i < n; i++)
      if (stored(i) && !A.iinit[i]) touch(i, NS * A.capP[i], -1);   // (the initial partials written up front)
    for (int k = 0; k < nst; k++) {
      if (!A.inpart(k)) continue;
      const int t = A.type(k), f0 = A.from0(k), f1 = A.from1(k), t0 = A.to0(k), sl = A.slot(k);
      if (stored(f0)) touch(f0, NS * A.capP[f0], ph[k]);
      if (t == 3 && stored(f1)) touch(f1, NS * A.capP[f1], ph[k]);
      if (t != 1 && stored(t0)) touch(t0, NS * A.capP[t0], ph[k]);
      if (sl != 255 && !A.leafs.count(sl)) touch(1000 + sl, msize(sl), ph[k]);
      if (t == 3) touch(-1, tmp, ph[k]);
    }
    const int fin_ = A.to0(nst - 1);
    if (stored(fin_)) touch(fin_, NS * A.capP[fin_], cur + 1);
    // first fit over a few placement orders (the first write, the size, the live-range length; ties by the others),
    // keeping the smallest footprint
    std::vector<int> ids;
    for (auto& r : rg) ids.push_back(r.first);
    auto fit = [&](const std::vector<int>& order, bool commit) {
      std::vector<std::pair<int, int>> pl;   // (id, offset)
      int t_ = LSZ;
      for (int id : order) {
        const Reg& r = rg[id];
        int o = LSZ;
        for (bool moved = true; moved;) {
          moved = false;
          for (auto& q : pl) {
            const Reg& a = rg[q.first];
            const bool live = a.hi >= r.lo && r.hi >= a.lo;
            if (live && o < q.second + a.size && q.second < o + r.size) { o = q.second + a.size; moved = true; }
          }
        }
        pl.push_back({id, o});
        t_ = std::max(t_, o + r.size);
      }
      if (commit)
        for (auto& q : pl) rg[q.first].off = q.second;
      return t_;
    };
    std::vector<std::vector<int>> orders;
    for (int key = 0; key < 3; key++) {
      std::vector<int> o = ids;
      std::stable_sort(o.begin(), o.end(), [&](int a, int b) {
        const Reg &x = rg[a], &y = rg[b];
        if (key == 0 && x.lo != y.lo) return x.lo < y.lo;
        if (key == 2 && x.hi - x.lo != y.hi - y.lo) return x.hi - x.lo > y.hi - y.lo;
        if (x.size != y.size) return x.size > y.size;
        return x.lo < y.lo;
      });
      orders.push_back(o);
    }
    size_t best = 0;
    int top_ = fit(orders[0], false);
    for (size_t q = 1; q < orders.size(); q++) {
      const int t_ = fit(orders[q], false);
      if (t_ < top_) { top_ = t_; best = q; }
    }
    fit(orders[best], true);
    for (auto& a : rg)   // (the invariant the placement keeps: regions live in a common phase never share a double)
      for (auto& b : rg)
        if (a.first < b.first && a.second.hi >= b.second.lo && b.second.hi >= a.second.lo &&
            a.second.off < b.second.off + b.second.size && b.second.off < a.second.off + a.second.size) {
          fprintf(stderr, "es_jit: workspace regions %d and %d overlap while live (%s)\n", a.first, b.first, A.name.c_str());
          abort();
        }
    for (auto& r : rg) {
      if (r.first == -1) A.TB = r.second.off;
      else if (r.first >= 1000) A.mo[r.first - 1000] = r.second.off;
      else A.po[r.first] = r.second.off;
    }
    if (!rg.count(-1)) A.TB = top_;   // (no type-3 step: tmp = 1, above the rest)
    A.NSZ = std::max(1, (rg.count(-1) ? top_ : top_ + tmp) - LSZ);
  }
  A.ws = part == 1 ? LSZ : LSZ + A.NSZ;   // (the leaf prefix writes its own regions only)
}

WaveFamily analyse_wave_family(const Family& F, int chrom, int NS, bool top, const std::string& name, int part, const Opts& opt) {
  WaveFamily A{F, chrom, NS, top, part, name, F.n, (int)F.steps.size()};
  const int n = A.n, nst = A.nst;
  // degrees through the peel (poly_layout's rule), capacities, temporaries (type 3 only: the W(i, j) products)
  A.d0.assign(n, 0); A.dP.assign(n, 0); A.capP.assign(n, 0);
  std::map<int, int> dM;
  const bool sp3_on = NS == 10 && opt.sp3;   // founder-sparse type-3 steps (see emit_type3_sparse)
  for (int pass = (part && top) ? 0 : 1; pass < 2; pass++) {   // (pass 0: the 10-state variant's capacities)
    const bool tp = pass == 1 && top;
    A.sd.clear(); dM.clear();
    for (int i = 0; i < n; i++) {
      A.d0[i] = A.dP[i] = (tp || !A.founder(i)) ? 0 : A.fdeg(i);
      A.capP[i] = std::max(pass ? A.capP[i] : 0, A.dP[i] + 1);
    }
    for (int k = 0; k < nst; k++) {
      const int type = A.type(k), from0 = A.from0(k), from1 = A.from1(k), to0 = A.to0(k), slot = A.slot(k);
      std::vector<int>& dP = A.dP;
      StepDeg g{0, 0, 0, 0};
      if (type == 1) {
        g.a = dP[from0]; g.b = A.create(k) ? 0 : dM[slot];
        dM[slot] = g.a + g.b;
        A.capM[slot] = std::max(A.capM[slot], dM[slot] + 1);
      } else if (type == 2) {
        g.a = dP[from0]; g.b = slot == 255 ? 0 : dM[slot]; g.c = dP[to0];
        dP[to0] = g.a + g.b + g.c;
        A.capP[to0] = std::max(A.capP[to0], dP[to0] + 1);
      } else {
        g.a = dP[from0]; g.b = slot == 255 ? 0 : dM[slot]; g.c = dP[from1]; g.e = dP[to0];
        dP[to0] = g.a + g.b + g.c + g.e;
        A.capP[to0] = std::max(A.capP[to0], dP[to0] + 1);
        // (the W(i, j) products: a founder-sparse step keeps only its supports' pairs; pterms' sizes)
        auto supp = [&](int f) {
          if (!(sp3_on && A.founder(f))) return NS;
          return top ? (A.fdeg(f) > 0 ? 1 : 3) : A.fdeg(f) == 1 ? 2 : 3;
        };
        A.tmp = std::max(A.tmp, supp(from0) * supp(from1) * (g.a + g.b + g.c + 1));
      }
      A.sd.push_back(g);
    }
  }
  A.sp3.assign(nst, 0);
  for (int k = 0; k < nst && sp3_on; k++)
    if (A.type(k) == 3 && (A.founder(A.from0(k)) || A.founder(A.from1(k)))) A.sp3[k] = 1;
  classify_steps(A);
  layout_workspace(A);
  if (opt.layout) {
    fprintf(stderr, "layout %s NS %d part %d top %d: LSZ %d NSZ %d tmp %d ws %d |", name.c_str(), NS, part, (int)top, A.LSZ, A.NSZ, A.tmp, A.ws);
    for (int i = 0; i < n; i++) fprintf(stderr, " p%d:%d%s", i, !A.penf[i] ? NS * A.capP[i] : 0, A.leafp[i] ? "L" : "");
    for (auto& m : A.capM) fprintf(stderr, " m%d:%d", m.first, A.mrows(m.first) * m.second);
    fprintf(stderr, " | offsets");
    for (int i = 0; i < n; i++) fprintf(stderr, " p%d@%d", i, A.po[i]);
    for (auto& m : A.capM) fprintf(stderr, " m%d@%d", m.first, A.mo[m.first]);
    fprintf(stderr, " tb@%d\n", A.TB);
  }
  return A;
}

// Emission: one function per phase kind, appending to the device function's text.  Every phase ends in a wave_sync.

// a phase with the family's lanes over index var < N
std::string lanes(int N, const std::string& var, const std::string& body) {
  return "  for (int " + var + " = lane; " + var + " < " + S(N) + "; " + var + " += " + S(kWl) + ") {\n" + body + "  }\n";
}
// a phase with the family's lanes over the NS x NS pairs e
std::string pair_lanes(const WaveFamily& A, const std::string& body) {
  return "#pragma unroll\n  for (int r = 0; r < " + S((A.NS * A.NS + kWl - 1) / kWl) + "; r++) {\n    const int e = lane + " + S(kWl) +
         " * r;\n    if (e < " + S(A.NS * A.NS) + ") {\n" + body + "    }\n  }\n  wave_sync();\n";
}
// coefficient a of the product of the register polynomials x (degree dx) and y (degree dy)
std::string conv(const std::string& x, int dx, const std::string& y, int dy, int a) {
  std::string acc;
  for (int c = std::max(0, a - dy); c <= std::min(a, dx); c++)
    acc = acc.empty() ? x + "[" + S(c) + "] * " + y + "[" + S(a - c) + "]" : "fma(" + x + "[" + S(c) + "], " + y + "[" + S(a - c) + "], " + acc + ")";
  return acc;
}
// T(e = i NS + j, k) of an offspring: the 10-state tables (the de novo transmission; the plain one, quirk :1391) from
// global memory, the bi-allelic class tables in LDS
std::string tt(const WaveFamily& A, int csex, const std::string& e, const std::string& k, bool plain) {
  if (A.NS == 10) return plain ? "t10[(" + e + ") * 10 + " + k + "]" : "t10dn[(" + e + ") * 10 + " + k + "]";
  const int t = A.chrom == PM_CHR_X ? (csex == MALE ? 2 : 1) : A.chrom == PM_CHR_Y ? (csex == MALE ? 3 : 5) : A.chrom == PM_CHR_MT ? 4 : 0;
  return "tb[" + S(t * 27) + " + (" + e + ") * 3 + " + k + "]";
}

// InitializePartials x SetFounderPriors, one person at a time (lanes over its states); persons without a region
// (penf, penp) and those whose type-2 step forms the initial partial (iinit) are skipped
void emit_initial_partials(const WaveFamily& A, std::string& code) {
  const int n = A.n, NS = A.NS;
  code += "  const int g11 = gg11, g12 = gg12, g22 = gg22;\n  (void)g11; (void)g12; (void)g22;\n";
  for (int i = 0; i < n; i++) {
    if ((A.part == 1 && !A.leafp[i]) || (A.part == 2 && A.leafp[i])) continue;
    if (A.penf[i] || A.iinit[i] || A.penp[i]) continue;
    const bool fo = A.founder(i);
    const bool yf = NS == 3 && A.chrom == PM_CHR_Y && A.F.sex[i] == FEMALE;
    const int dfull = !fo ? 0 : A.fdeg(i);
    const int d = A.d0[i];
    std::string b = "    const int o = " + A.PO(i) + " + x * " + S(A.capP[i]) + ";\n";
    for (int a = 0; a <= d; a++) b += "    W[o + " + S(a) + "] = 0.0;\n";
    if (NS == 3) {
      b += "    const double pen = PEN[(x == 0 ? g11 : x == 1 ? g12 : g22) * " + S(n) + " + " + S(i) + "];\n";
      if (yf) b += "    W[o] = 1.0;\n";
      else if (!fo) b += "    W[o] = pen;\n";
      else if (A.top) b += "    if (x == 0) W[o] = pen;\n";
      else if (d == 2) b += "    W[o + 2 - x] = x == 1 ? 2 * pen : pen;\n";
      else b += "    if (x != 1) W[o + (x == 0 ? 1 : 0)] = pen;\n";
    } else {
      b += "    const double pen = PEN[x * " + S(n) + " + " + S(i) + "];\n";
      b += "    const int q = x == g11 ? 0 : x == g12 ? 1 : x == g22 ? 2 : 3;\n    (void)q;\n";
      if (!fo) b += "    W[o] = pen;\n";
      else if (A.top && dfull > 0) b += "    if (q == 0) W[o] = pen;\n";
      else if (d == 2) b += "    if (q != 3) W[o + 2 - q] = q == 1 ? 2 * pen : pen;\n";
      else if (d == 1) b += "    if (q == 0 || q == 2) W[o + (q == 0 ? 1 : 0)] = pen;\n";
      else b += "    if (q != 3) W[o] = pen;\n";
    }
    code += lanes(NS, "x", b);
  }
  code += "  wave_sync();\n";
}

// A bi-allelic type-1 step k (peelOffspring2Parents_BA): lanes over the pairs e, S(e) = sum_k T(e, k) P_off[k] in
// registers, then M(e) *= S(e) in place
void emit_type1_step(const WaveFamily& A, int k, std::string& code) {
  const StepDeg g = A.sd[k];
  const int off_ = A.from0(k), csex = A.F.sex[off_], pcap = A.capP[off_], slot = A.slot(k);
  std::string b = "      double s[" + S(g.a + 1) + "];\n";
  for (int a = 0; a <= g.a; a++) {
    b += "      s[" + S(a) + "] = 0.0;\n";
    b += "#pragma unroll\n      for (int k = 0; k < " + S(A.NS) + "; k++) s[" + S(a) + "] = fma(" + tt(A, csex, "e", "k", false) + ", W[" +
         A.PO(off_) + " + k * " + S(pcap) + " + " + S(a) + "], s[" + S(a) + "]);\n";
  }
  const std::string me = A.MO(slot) + " + e * " + S(A.mcap(slot));
  if (A.create(k)) {
    for (int a = 0; a <= g.a; a++) b += "      W[" + me + " + " + S(a) + "] = s[" + S(a) + "];\n";
  } else {
    b += "      double m[" + S(g.b + 1) + "];\n";
    for (int c = 0; c <= g.b; c++) b += "      m[" + S(c) + "] = W[" + me + " + " + S(c) + "];\n";
    for (int a = 0; a <= g.a + g.b; a++) b += "      W[" + me + " + " + S(a) + "] = " + conv("m", g.b, "s", g.a, a) + ";\n";
  }
  code += pair_lanes(A, b);
}

// A run of consecutive 10-state type-1 steps (this part's; they only read offspring partials and their own marriage
// partial) is one phase: lanes over the pairs (lane, lane + 32, ... < 100), one pass over k for every step of the run
// (each offspring coefficient read from LDS once for the lane's pairs: wave-uniform broadcasts), then per marriage
// partial the steps' products chained in registers and one write -- the same operations in the same order as step by
// step.  sp: the run's founder-sparse rows (only the pairs of the founder's non-zero states are computed).
void emit_type1_run(const WaveFamily& A, const std::vector<int>& run, const Sparse& sp, std::string& code) {
  const int n = A.n;
  std::vector<int> slots;   // the marriage partials the run writes, in order of first use
  for (int k2 : run)
    if (std::find(slots.begin(), slots.end(), A.slot(k2)) == slots.end()) slots.push_back(A.slot(k2));
  const bool sparse = !sp.terms.empty();
  const int nsp = 10 * (int)sp.terms.size();   // (sparse: the rows, passes of kWl lanes over them)
  const int npair = sparse ? (nsp + kWl - 1) / kWl : (100 + kWl - 1) / kWl;
  std::string c1 = "  {\n";
  if (sparse) {   // pass pr: row p = lane + pr kWl (state o of the spouse, term qi of the founder's support); rows past
                  // the support compute an in-range pair and store nothing
    const std::string gq[3] = {"g11", "g12", "g22"};
    for (int pr = 0; pr < npair; pr++) {
      const std::string P = S(pr), qi = "qi" + P;
      std::string sF = gq[sp.terms.back().first];
      for (int q = (int)sp.terms.size() - 2; q >= 0; q--) sF = qi + " == " + S(q) + " ? " + gq[sp.terms[q].first] + " : " + sF;
      c1 += "    const int p" + P + " = lane + " + S(pr * kWl) + ", " + qi + " = p" + P + " / 10, o" + P + " = p" + P + " - " + qi +
            " * 10, sF" + P + " = " + sF + ";\n    const int e" + P + " = " +
            (sp.father ? "sF" + P + " * 10 + o" + P : "o" + P + " * 10 + sF" + P) + ";\n";
    }
  } else
    for (int pr = 1; pr < npair; pr++)
      c1 += "    const int e" + S(pr) + " = lane + " + S(pr * kWl) + ", e" + S(pr) + "c = e" + S(pr) + " < 100 ? e" + S(pr) + " : lane;\n";
  for (size_t q = 0; q < run.size(); q++) {
    const int ga = A.sd[run[q]].a;
    for (int pr = 0; pr < npair; pr++) {
      c1 += "    double s" + S(pr) + "_" + S(q) + "[" + S(ga + 1) + "];\n";
      for (int a = 0; a <= ga; a++) c1 += "    s" + S(pr) + "_" + S(q) + "[" + S(a) + "] = 0.0;\n";
    }
  }
  // (k unrolled by 2 only: fully unrolled, the scheduler hoists every offspring coefficient's LDS read and spills)
  c1 += "#pragma unroll 2\n    for (int k = 0; k < 10; k++) {\n";
  c1 += sparse ? "      const double t0 = t10dn[e0 * 10 + k]" : "      const double t0 = t10dn[lane * 10 + k]";   // the rows of this lane's pairs
  for (int pr = 1; pr < npair; pr++) c1 += ", t" + S(pr) + " = t10dn[e" + S(pr) + (sparse ? "" : "c") + " * 10 + k]";
  c1 += ";\n";
  for (size_t q = 0; q < run.size(); q++) {
    const int offq = A.from0(run[q]), ga = A.sd[run[q]].a;
    for (int a = 0; a <= ga; a++) {
      c1 += A.penp[offq] ? "      {\n        const double p = PEN[k * " + S(n) + " + " + S(offq) + "];\n"
                         : "      {\n        const double p = W[" + A.PO(offq) + " + k * " + S(A.capP[offq]) + " + " + S(a) + "];\n";
      for (int pr = 0; pr < npair; pr++)
        c1 += "        s" + S(pr) + "_" + S(q) + "[" + S(a) + "] = fma(t" + S(pr) + ", p, s" + S(pr) + "_" + S(q) + "[" + S(a) + "]);\n";
      c1 += "      }\n";
    }
  }
  c1 += "    }\n";
  // per pair: each marriage partial chained through its steps in registers, one write
  for (int pr = 0; pr < npair; pr++) {
    const std::string sq_ = "s" + S(pr) + "_", e = sp.compact ? "p" + S(pr) : sparse ? "e" + S(pr) : pr ? "e" + S(pr) : "lane";
    c1 += sparse ? "    if (p" + S(pr) + " < " + S(nsp) + ") {\n" : pr ? "    if (e" + S(pr) + " < 100) {\n" : "    {\n";
    int cid = 0;
    for (int sl2 : slots) {
      const std::string mev = A.MO(sl2) + " + " + e + " * " + S(A.mcap(sl2));
      std::string cur;   // the register array holding the slot's current coefficients
      int dcur = -1;
      for (size_t q = 0; q < run.size(); q++) {
        if (A.slot(run[q]) != sl2) continue;
        const int ga = A.sd[run[q]].a, gb = A.sd[run[q]].b;
        const std::string sq = sq_ + S(q);
        if (A.create(run[q])) { cur = sq; dcur = ga; continue; }
        if (dcur < 0) {   // the slot's coefficients so far, from LDS
          cur = "m" + S(pr) + "_" + S(cid++);
          c1 += "      double " + cur + "[" + S(gb + 1) + "];\n";
          for (int c = 0; c <= gb; c++) c1 += "      " + cur + "[" + S(c) + "] = W[" + mev + " + " + S(c) + "];\n";
          dcur = gb;
        }
        const std::string nx = "m" + S(pr) + "_" + S(cid++);
        c1 += "      double " + nx + "[" + S(ga + gb + 1) + "];\n";
        for (int a = 0; a <= ga + gb; a++) c1 += "      " + nx + "[" + S(a) + "] = " + conv(cur, gb, sq, ga, a) + ";\n";
        cur = nx;
        dcur = ga + gb;
      }
      for (int a = 0; a <= dcur; a++) c1 += "      W[" + mev + " + " + S(a) + "] = " + cur + "[" + S(a) + "];\n";
    }
    c1 += "    }\n";
  }
  code += c1 + "  }\n  wave_sync();\n";
}

// The independent type-2 steps of one shape that follow step k (this part's, 10 states): they share one phase, 16 lanes
// per step, the lane's step selecting its partials' offsets
std::vector<int> type2_run(const WaveFamily& A, int k) {
  std::vector<int> run{k};
  if (A.NS != 10) return run;
  auto sig2 = [&](int k2) {
    const int f2 = A.from0(k2), t2 = A.to0(k2), s2 = A.slot(k2);
    return std::vector<int>{A.pristine[k2], A.sd[k2].a, A.sd[k2].b, A.sd[k2].c, s2 == 255, A.capP[f2], A.capP[t2], s2 == 255 ? 0 : A.mcap(s2),
                            A.d0[f2], (int)A.crows.count(s2), (int)A.penf[f2], (int)A.iinit[t2], A.founder(t2),
                            A.founder(t2) ? A.fdeg(t2) : -1};
  };
  const std::vector<int> sg0 = sig2(k);
  for (int k2 = k + 1; k2 < A.nst && (int)run.size() < kWl / 16; k2++) {
    if (!A.inpart(k2)) continue;
    if (A.type(k2) != 2 || sig2(k2) != sg0) break;
    const int f2 = A.from0(k2), t2 = A.to0(k2);
    bool indep = true;
    for (int k3 : run)
      if (t2 == A.to0(k3) || f2 == A.to0(k3) || A.from0(k3) == t2) indep = false;
    if (!indep) break;
    run.push_back(k2);
  }
  return run;
}

// Type-2 step run[0], or the packed run of type2_run (peelSpouse2Spouse_BA): lanes over i, S(i) = sum_j P_from[j]
// M(j, i) in registers, then P_to[i] *= S(i) in place
void emit_type2(const WaveFamily& A, const std::vector<int>& run, std::string& code) {
  const int kstep = run[0], n = A.n, NS = A.NS;
  const StepDeg g = A.sd[kstep];
  const int sf = A.from0(kstep), stt = A.to0(kstep), slot = A.slot(kstep), fcap = A.capP[sf], tcap = A.capP[stt];
  const int ds = g.a + g.b;
  const bool packed = run.size() > 1;
  const std::string nsS = S(NS);
  // q_ == 0 ? f(run[0]) : ... : f(run.back()): the value of the lane group's step
  auto sel = [&](const std::function<std::string(int)>& f) {
    std::string e = f(run.back());
    for (int q = (int)run.size() - 2; q >= 0; q--) e = "q_ == " + S(q) + " ? " + f(run[q]) + " : " + e;
    return e;
  };
  std::string OF = A.PO(sf), OT = A.PO(stt), OM = slot == 255 ? "" : A.MO(slot), pre;
  if (packed) {
    pre = "      const int of_ = " + sel([&](int k2) { return A.PO(A.from0(k2)); }) +
          ";\n      const int ot_ = " + sel([&](int k2) { return A.PO(A.to0(k2)); }) + ";\n";
    if (slot != 255) {   // (and the marriage partial's orientation: M(i, j) or M(j, i))
      pre += "      const int om_ = " + sel([&](int k2) { return A.MO(A.slot(k2)); }) + ";\n";
      pre += "      const int si_ = " + sel([&](int k2) { return std::string(A.fa2mo(k2) ? "1" : nsS); }) + ", sj_ = " +
             sel([&](int k2) { return std::string(A.fa2mo(k2) ? nsS : "1"); }) + ";\n";
    }
    OF = "of_"; OT = "ot_"; OM = "om_";
  }
  const std::string me = packed ? "(i * si_ + j * sj_)" : A.fa2mo(kstep) ? "(j * " + nsS + " + i)" : "(i * " + nsS + " + j)";

  std::string b = "    double s[" + S(ds + 1) + "];\n";
  for (int a = 0; a <= ds; a++) b += "    s[" + S(a) + "] = 0.0;\n";
  if (A.pristine[kstep]) {
    // the founder's partial is prior x penetrance: state g11 / g12 / g22 holds one monomial, at coefficient
    // 2 - q (degree 2: q = 0, 1, 2), 1 / - / 0 (degree 1: no geno12) or 0 (degree 0); the other states are zero.
    // The sum visits j in the dense loop's order and skips the zero terms (fma(0, g, s) == s), so it is
    // bit-identical to the dense sum (q in the dense loop's coefficient order u = 0, 1, 2 at one j, should two of
    // the genotypes coincide)
    // No loop over j: the terms' states are wave-uniform, so their order by j (stable: ties keep the coefficient
    // order) is one of at most 6, chosen once by a uniform switch; each case adds the terms in that order
    const std::string gq[3] = {"g11", "g12", "g22"};
    const std::vector<std::pair<int, int>> tm = A.pterms(sf);
    auto term = [&](int q, int u, int qpos) {
      std::string t = "      {\n        const int j = " + gq[q] + ";\n";
      if (A.penf[sf]) {   // the penetrance the init phase would have stored, from PEN (one read: the person index selected;
                          // x 2 for the heterozygote's coefficient)
        t += "        const double pj_ = PEN[j * " + S(n) + " + (" + sel([&](int k2) { return S(A.from0(k2)); }) + ")];\n";
        t += (!A.top && A.d0[sf] == 2 && q == 1) ? "        const double f = 2 * pj_;\n" : "        const double f = pj_;\n";
      } else t += "        const double f = W[" + OF + " + j * " + S(fcap) + " + " + S(u) + "];\n";
      if (slot == 255) t += "        s[" + S(u) + "] += f;\n";
      else {
        const std::string mr = A.crows.count(slot) ? "(" + S(qpos * 10) + " + i)" : me;   // (compact rows)
        for (int v = 0; v <= g.b; v++)
          t += "        s[" + S(u + v) + "] = fma(f, W[" + OM + " + " + mr + " * " + S(A.mcap(slot)) + " + " + S(v) + "], s[" + S(u + v) + "]);\n";
      }
      return t + "      }\n";
    };
    const int nt = (int)tm.size();
    if (nt == 1) b += term(tm[0].first, tm[0].second, 0);
    else {
      // bit c of the case: term a (of pair c) is not after term b, in the terms' order a < b
      std::vector<std::pair<int, int>> prs;
      for (int a = 0; a < nt; a++)
        for (int c = a + 1; c < nt; c++) prs.push_back({a, c});
      std::string key;
      for (size_t c = 0; c < prs.size(); c++)
        key += std::string(c ? " | " : "") + "((" + gq[tm[prs[c].first].first] + " <= " + gq[tm[prs[c].second].first] + ") << " + S(c) + ")";
      b += "    switch (" + key + ") {\n";
      for (int cs = 0; cs < (1 << prs.size()); cs++) {
        std::vector<int> ord(nt);
        for (int a = 0; a < nt; a++) ord[a] = a;
        auto before = [&](int x, int y) {   // x before y in this case
          for (size_t c = 0; c < prs.size(); c++) {
            if (prs[c].first == x && prs[c].second == y) return ((cs >> c) & 1) != 0;
            if (prs[c].first == y && prs[c].second == x) return ((cs >> c) & 1) == 0;
          }
          return x < y;
        };
        std::stable_sort(ord.begin(), ord.end(), before);
        b += "      case " + S(cs) + ":\n";
        for (int a : ord) b += term(tm[a].first, tm[a].second, a);
        b += "      break;\n";
      }
      b += "    }\n";
    }
  } else if (slot == 255) {
    for (int a = 0; a <= ds; a++)
      b += "#pragma unroll\n    for (int j = 0; j < " + nsS + "; j++) s[" + S(a) + "] += W[" + OF + " + j * " + S(fcap) + " + " +
           S(a) + "];\n";
  } else {
    b += std::string(packed ? "#pragma unroll 2" : "#pragma unroll") + "\n    for (int j = 0; j < " + nsS + "; j++) {\n";
    for (int u = 0; u <= g.a; u++) b += "      const double f" + S(u) + " = W[" + OF + " + j * " + S(fcap) + " + " + S(u) + "];\n";
    for (int v = 0; v <= g.b; v++) b += "      const double g" + S(v) + " = W[" + OM + " + " + me + " * " + S(A.mcap(slot)) + " + " + S(v) + "];\n";
    for (int u = 0; u <= g.a; u++)
      for (int v = 0; v <= g.b; v++) b += "      s[" + S(u + v) + "] = fma(f" + S(u) + ", g" + S(v) + ", s[" + S(u + v) + "]);\n";
    b += "    }\n";
  }
  b += "    double t[" + S(g.c + 1) + "];\n";
  if (A.iinit[stt]) {   // the initial partial at state i (InitializePartials x SetFounderPriors), of the lane group's to-person
    const bool fo2 = A.founder(stt);
    const int dfull2 = !fo2 ? 0 : A.fdeg(stt);
    const int d2 = A.d0[stt];
    b += "    const double pen_ = PEN[i * " + S(n) + " + (" + sel([&](int k2) { return S(A.to0(k2)); }) + ")];\n";
    b += "    const int qi_ = i == g11 ? 0 : i == g12 ? 1 : i == g22 ? 2 : 3;\n    (void)qi_;\n";
    for (int c = 0; c <= g.c; c++) {
      std::string v = "0.0";
      if (!fo2) v = c == 0 ? "pen_" : "0.0";
      else if (A.top && dfull2 > 0) v = c == 0 ? "(qi_ == 0 ? pen_ : 0.0)" : "0.0";
      else if (d2 == 2) v = c == 0 ? "(qi_ == 2 ? pen_ : 0.0)" : c == 1 ? "(qi_ == 1 ? 2 * pen_ : 0.0)" : c == 2 ? "(qi_ == 0 ? pen_ : 0.0)" : "0.0";
      else if (d2 == 1) v = c == 0 ? "(qi_ == 2 ? pen_ : 0.0)" : c == 1 ? "(qi_ == 0 ? pen_ : 0.0)" : "0.0";
      else v = c == 0 ? "(qi_ != 3 ? pen_ : 0.0)" : "0.0";
      b += "    t[" + S(c) + "] = " + v + ";\n";
    }
  } else
    for (int c = 0; c <= g.c; c++) b += "    t[" + S(c) + "] = W[" + OT + " + i * " + S(tcap) + " + " + S(c) + "];\n";
  for (int a = 0; a <= g.c + ds; a++) b += "    W[" + OT + " + i * " + S(tcap) + " + " + S(a) + "] = " + conv("t", g.c, "s", ds, a) + ";\n";
  if (packed)
    code += "  {\n    const int q_ = lane >> 4, i = lane & 15;\n    if (q_ < " + S(run.size()) + " && i < " + nsS + ") {\n" + pre + b +
            "    }\n  }\n  wave_sync();\n";
  else code += lanes(NS, "i", b) + "  wave_sync();\n";
}

// the second half of a type-3 step: lanes over the child states k, P_off[k] *= S(k), S(k) = the sum `loop` accumulates
// into s[] over the products at W[TB + ...]
void emit_type3_child(const WaveFamily& A, int k, const std::string& loop, std::string& code) {
  const StepDeg g = A.sd[k];
  const int off_ = A.to0(k), dw = g.a + g.b + g.c;
  std::string b2 = "    double s[" + S(dw + 1) + "];\n";
  for (int a = 0; a <= dw; a++) b2 += "    s[" + S(a) + "] = 0.0;\n";
  b2 += loop + "    }\n    double t[" + S(g.e + 1) + "];\n";
  for (int c = 0; c <= g.e; c++) b2 += "    t[" + S(c) + "] = W[" + A.PO(off_) + " + k * " + S(A.capP[off_]) + " + " + S(c) + "];\n";
  for (int a = 0; a <= g.e + dw; a++)
    b2 += "    W[" + A.PO(off_) + " + k * " + S(A.capP[off_]) + " + " + S(a) + "] = " + conv("t", g.e, "s", dw, a) + ";\n";
  code += lanes(A.NS, "k", b2) + "  wave_sync();\n";
}
// the first half: w = P_fa[i] M(e) P_mo[j] of the lane's pair (i, j, e) into W[TB + at * (dw + 1) ...]
std::string type3_products(const WaveFamily& A, int k, const std::string& at) {
  const StepDeg g = A.sd[k];
  const int fa = A.from0(k), mo_ = A.from1(k), slot = A.slot(k), dw = g.a + g.b + g.c, ww = dw + 1;
  std::string b = "      double w[" + S(ww) + "];\n";
  for (int a = 0; a <= dw; a++) b += "      w[" + S(a) + "] = 0.0;\n";
  for (int u = 0; u <= g.a; u++)
    for (int v = 0; v <= g.b; v++)
      for (int c = 0; c <= g.c; c++) {
        const std::string m = slot == 255 ? "" : " * W[" + A.MO(slot) + " + e * " + S(A.mcap(slot)) + " + " + S(v) + "]";
        b += "      w[" + S(u + v + c) + "] = fma(W[" + A.PO(fa) + " + i * " + S(A.capP[fa]) + " + " + S(u) + "]" + m + ", W[" +
             A.PO(mo_) + " + j * " + S(A.capP[mo_]) + " + " + S(c) + "], w[" + S(u + v + c) + "]);\n";
      }
  for (int a = 0; a <= dw; a++) b += "      W[" + S(A.TB) + " + " + at + " * " + S(ww) + " + " + S(a) + "] = w[" + S(a) + "];\n";
  return b;
}

// Dense type-3 step k (peelParents2Offspring_BA): W(e) = P_fa[i] M(e) P_mo[j] -> LDS; lanes over k: S(k) = sum_e T(e, k)
// W(e), P_off[k] *= S(k) in place.  Returns whether the step reads the LDS list t3z / t3n.
bool emit_type3_dense(const WaveFamily& A, int k, const Opts& opt, std::string& code) {
  const StepDeg g = A.sd[k];
  const int csex = A.F.sex[A.to0(k)], slot = A.slot(k), ww = g.a + g.b + g.c + 1;
  const std::string nsS = S(A.NS);
  code += pair_lanes(A, "      const int i = e / " + nsS + ", j = e - i * " + nsS + ";\n" + type3_products(A, k, "e"));
  // 10 states, with a marriage partial: the plain transmission (:1391) is the Mendelian table, 16-31 of a child state's
  // 100 parent pairs are non-zero (1, 1/2 or 1/4).  Each lane k runs over its non-zero pairs only, in ascending e (the
  // LDS list t3z, e << 2 | value code, filled from kT3z / kT3n at kernel start): the pairs skipped would add +0 (T = 0, W
  // finite and >= 0), so every sum keeps its bits -- and no transmission load is waited for in the 100-step loop
  const bool t3z = A.NS == 10 && slot != 255 && opt.t3z;
  std::string loop = t3z ? "    const int nz_ = t3n[k];\n    for (int q_ = 0; q_ < nz_; q_++) {\n      const int pk_ = t3z[k * 32 + q_], e = pk_ >> 2;\n"
                           "      const double t = (pk_ & 3) == 0 ? 1.0 : (pk_ & 3) == 1 ? 0.5 : 0.25;\n"
                         : "    for (int e = 0; e < " + S(A.NS * A.NS) + "; e++) {\n      const double t = " + tt(A, csex, "e", "k", slot != 255) + ";\n";
  for (int a = 0; a < ww; a++) loop += "      s[" + S(a) + "] = fma(t, W[" + S(A.TB) + " + e * " + S(ww) + " + " + S(a) + "], s[" + S(a) + "]);\n";
  emit_type3_child(A, k, loop, code);
  return t3z;
}

// Founder-sparse type-3 step k (10 states): a founder's partial is prior x penetrance times whatever multiplied into
// it -- zero outside the 1-3 states of its prior (the site's g11, g12, g22; pterms) -- so W(e) = P_fa[i] M(e) P_mo[j]
// is zero off those pairs, and so is every term T(e, k) W(e) they would add (+0: the sums keep their bits).  Only
// the nI x nJ pairs (i, j) in ascending e are formed (lanes over them) and summed (in the same ascending e order),
// instead of all 100.  The states of a founder's support are sorted at run time (wave-uniform).
void emit_type3_sparse(const WaveFamily& A, int k, std::string& code) {
  const StepDeg g = A.sd[k];
  const int csex = A.F.sex[A.to0(k)], slot = A.slot(k), ww = g.a + g.b + g.c + 1;
  const std::string nsS = S(A.NS);
  auto support = [&](int f, const std::string& pre) -> std::pair<int, std::string> {
    if (!A.founder(f)) return {10, ""};
    const auto t = A.pterms(f);
    std::string c;
    for (size_t q = 0; q < t.size(); q++)
      c += "  int " + pre + S(q) + " = " + (t[q].first == 0 ? "g11" : t[q].first == 1 ? "g12" : "g22") + ";\n";
    auto sw = [&](int a, int b2) {
      return "  if (" + pre + S(a) + " > " + pre + S(b2) + ") { const int x_ = " + pre + S(a) + "; " + pre + S(a) + " = " + pre + S(b2) +
             "; " + pre + S(b2) + " = x_; }\n";
    };
    if (t.size() >= 2) c += sw(0, 1);
    if (t.size() == 3) c += sw(1, 2) + sw(0, 1);
    return {(int)t.size(), c};
  };
  const std::string pI = "sI" + S(k) + "_", pJ = "sJ" + S(k) + "_";
  const auto sI = support(A.from0(k), pI), sJ = support(A.from1(k), pJ);
  const int nI = sI.first, nJ = sJ.first, NP = nI * nJ;
  auto pick = [&](const std::string& pre, int nn, const std::string& idx) {   // the idx-th state of a support
    if (nn == 10) return idx;
    std::string r = pre + S(nn - 1);
    for (int q = nn - 2; q >= 0; q--) r = "(" + idx + " == " + S(q) + " ? " + pre + S(q) + " : " + r + ")";
    return r;
  };
  code += sI.second + sJ.second;
  const std::string b = "      const int ia = p / " + S(nJ) + ", jb = p - ia * " + S(nJ) + ";\n      const int i = " + pick(pI, nI, "ia") +
                        ", j = " + pick(pJ, nJ, "jb") + ", e = i * " + nsS + " + j;\n" + type3_products(A, k, "p");
  code += "#pragma unroll\n  for (int r = 0; r < " + S((NP + kWl - 1) / kWl) + "; r++) {\n    const int p = lane + " + S(kWl) + " * r;\n    if (p < " +
          S(NP) + ") {\n" + b + "    }\n  }\n  wave_sync();\n";
  std::string loop = "    for (int p = 0; p < " + S(NP) + "; p++) {\n      const int ia = p / " + S(nJ) + ", jb = p - ia * " + S(nJ) + ";\n      const int e = " +
                     pick(pI, nI, "ia") + " * " + nsS + " + " + pick(pJ, nJ, "jb") + ";\n      const double t = " + tt(A, csex, "e", "k", slot != 255) + ";\n";
  for (int a = 0; a < ww; a++) loop += "      s[" + S(a) + "] = fma(t, W[" + S(A.TB) + " + p * " + S(ww) + " + " + S(a) + "], s[" + S(a) + "]);\n";
  emit_type3_child(A, k, loop, code);
}

// CalculateLikelihood_BA: the final person's partials summed over the states, one lane per coefficient, and the degree word
void emit_final_sum(const WaveFamily& A, int fin, std::string& code) {
  const int D = A.dP[fin];
  code += lanes(D + 1, "a", "    double s = 0.0;\n#pragma unroll\n    for (int i = 0; i < " + S(A.NS) + "; i++) s += W[" + A.PO(fin) + " + i * " +
                                S(A.capP[fin]) + " + a];\n    out[(size_t)a * os] = s;\n");
  code += "  if (lane < 1) out[(size_t)(dcap - 1) * os] = " + S(D) + ".0;\n  wave_sync();\n";
}

// The device function of an analysed family: the phases in schedule order.  ops: the FP64 operations the generated
// phases perform (summed over their work elements: the useful lane-operations, whatever the lanes' occupancy);
// *uses_t3z is set when a phase reads the Mendelian LDS list.
std::string emit_wave_family(const WaveFamily& A, const Opts& opt, double* ops, bool* uses_t3z) {
  const int nst = A.nst, NS = A.NS;
  std::string code;
  emit_initial_partials(A, code);
  double nops = 0, lane_slots = 0;
  std::vector<char> done(nst, 0);         // steps emitted with the first step of their run
  std::vector<double> eff2(nst, 0.0);     // packed type-2 runs: the run's lane occupancy (10 r of kWl lanes)
  std::vector<double> frac1(nst, 1.0);    // type-1 steps: the fraction of the 100 pairs computed (founder-sparse rows)
  for (int k = 0; k < nst; k++) {
    if (!A.inpart(k)) continue;
    const StepDeg g = A.sd[k];
    const int type = A.type(k), slot = A.slot(k);
    // this step's FP64 operations (per item), and the lane slots they occupy (PM_JIT_LAYOUT: the static lane
    // occupancy -- a phase over E elements on a family's kWl lanes runs ceil(E / kWl) passes of kWl lanes; a packed
    // run of r type-2 steps fills 10 r of the kWl lanes; PM_JIT_STEPS: per step)
    const double ns = NS, before = nops;
    auto occ = [&](double E, double lanes) { return E / (std::ceil(E / lanes) * lanes); };
    auto ops1 = [&](double pairs) { return pairs * ((g.a + 1) * ns + (A.create(k) ? 0 : (g.a + 1) * (g.b + 1))); };
    double eff = 1.0;
    if (type == 1) {
      nops += ops1(frac1[k] * ns * ns);
      eff = occ(frac1[k] * ns * ns, kWl);
    } else if (type == 2) {
      const int ds = g.a + g.b;
      if (A.pristine[k]) nops += ns * ((double)A.pterms(A.from0(k)).size() * (slot == 255 ? 1 : (g.b + 1)) + (g.c + 1) * (ds + 1));
      else nops += ns * ((slot == 255 ? (ds + 1) * ns : ns * (g.a + 1) * (g.b + 1)) + (g.c + 1) * (ds + 1));
      eff = eff2[k] > 0 ? eff2[k] : occ(ns, kWl);   // (a packed run's first step: corrected below)
    } else {
      const int dw = g.a + g.b + g.c;
      double np_ = ns * ns;   // (founder-sparse: the pairs of the founders' supports only)
      if (A.sp3[k]) {
        const int f0 = A.from0(k), f1 = A.from1(k);
        np_ = (double)(A.founder(f0) ? (int)A.pterms(f0).size() : 10) * (A.founder(f1) ? (int)A.pterms(f1).size() : 10);
      }
      const double o1 = np_ * (g.a + 1) * (g.b + 1) * (g.c + 1) * (slot == 255 ? 1 : 2), o2 = ns * (np_ * (dw + 1) + (g.e + 1) * (dw + 1));
      nops += o1 + o2;
      eff = (o1 + o2) / (o1 / occ(np_, kWl) + o2 / occ(ns, kWl));
    }
    lane_slots += (nops - before) / eff;
    const double step_ops = nops - before;
    if (opt.steps)
      fprintf(stderr, "  step %s part %d M 1 k %d type %d ops %.0f eff %.3f\n", A.name.c_str(), A.part, k, type, step_ops, eff);
    if (done[k]) continue;
    if (type == 1 && NS == 10) {
      const std::vector<int> run = A.run_of(k);
      const Sparse sp = A.sparse_of(run);
      for (int k2 : run) done[k2] = 1;
      if (!sp.terms.empty()) {   // (this step, the run's first, was counted at 100 pairs above)
        const double fr = 10.0 * sp.terms.size() / 100.0;
        nops -= ops1((1.0 - fr) * 100.0);
        for (int k2 : run) frac1[k2] = fr;
      }
      emit_type1_run(A, run, sp, code);
    } else if (type == 1) emit_type1_step(A, k, code);
    else if (type == 2) {
      const std::vector<int> run = type2_run(A, k);
      if (run.size() > 1) {
        for (int k2 : run) { eff2[k2] = (double)NS * run.size() / kWl; done[k2] = 1; }
        lane_slots += step_ops / eff2[k] - step_ops / eff;
      }
      emit_type2(A, run, code);
    } else if (A.sp3[k]) emit_type3_sparse(A, k, code);
    else if (emit_type3_dense(A, k, opt, code)) *uses_t3z = true;
  }
  const int fin = A.to0(nst - 1);
  *ops = nops + (A.part == 1 ? 0.0 : (double)(A.dP[fin] + 1) * NS);
  if (opt.layout)
    fprintf(stderr, "occupancy %s part %d WL %d: %.0f FP64 ops / %.0f lane slots = %.3f\n", A.name.c_str(), A.part, kWl, nops, lane_slots,
            lane_slots > 0 ? nops / lane_slots : 0.0);
  if (A.part != 1) emit_final_sum(A, fin, code);
  // (tr0 / tr1: arguments the functions no longer read; the kernel text is pinned, see tests/test_cpu_jit_source.py)
  return "__device__ __forceinline__ void " + A.name +
         "(const uint8_t* __restrict__ pl, size_t np, const uint8_t* __restrict__ P11, const uint8_t* __restrict__ P12, "
         "const uint8_t* __restrict__ P22, int p0, int gg11, int gg12, int gg22, const double* lk, const double* __restrict__ t10, "
         "const double* __restrict__ t10dn, const double* tb, const double* tr0, const double* tr1, double* W, int lane, "
         "double* __restrict__ out, int os, int dcap, size_t ostr, const double* PEN) {\n" + code + "}\n";
}

// The site's penetrances of a family, lk[pl[g][p0 + i]] for the 10 genotypes g, into the family's LDS table PEN[g * n + i]
// (one coalesced pass per (site, family) instead of a dependent global load per person and variant)
std::string gen_pen_fill(int n, const std::string& name) {
  const std::string N = std::to_string(n);
  return "__device__ __forceinline__ void " + name + "(const uint8_t* __restrict__ pl, size_t np, int p0, const double* lk, double* PEN, "
         "int lane) {\n  for (int e = lane; e < " + std::to_string(10 * n) + "; e += " + std::to_string(kWl) + ") {\n    const int g = e / " + N + ", i = e - g * " + N +
         ";\n    PEN[e] = lk[pl[(size_t)g * np + p0 + i]];\n  }\n  wave_sync();\n}\n";
}

// fns: 3 variants per shape (bi-allelic, 10-state, top); parts: 3 per shape, the 10-state leaf prefix, the 10-state rest
// and the top variant's rest.
// The kernel's text is pinned byte for byte (tests/test_cpu_jit_source.py): a few of its lines still show what earlier
// switches substituted (`true &&`, `(true:`, `if (false && ...)`, the unused tr0 / tr1 rows) -- dead text the compiler
// drops, to go with the next change that is meant to alter the kernels.
std::string gen_wave_kernel(const std::vector<std::string>& fns, const std::vector<std::string>& parts, const std::vector<std::string>& pens,
                            const std::vector<int>& shape_ns, int ws, int pensz, int wpb, bool parts_only, bool uses_t3z, const Opts& opt) {
  // prefetch registers per lane (0: families too large; up to 4)
  const int npf = pensz <= 4 * kWl ? (pensz + kWl - 1) / kWl : 0;
  // wave_sync: the phases' LDS hand-over inside one wave.  A wave's LDS instructions execute in issue order, so a
  // read after a write sees it without waiting for the write; only the compiler must not move accesses across:
  // wavefront-scope release / acquire fences, which wait for the outstanding LDS accesses (measured 2% faster than a
  // bare barrier with a compiler memory clobber, r05nf)
  std::string s = R"(
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
)";
  s += "__device__ __forceinline__ int shape_n(int sig) {\n  switch (sig) {\n";
  for (size_t i = 0; i < shape_ns.size(); i++) s += "    case " + std::to_string(i) + ": return " + std::to_string(shape_ns[i]) + ";\n";
  s += "  }\n  return 0;\n}\n";
  std::string k = R"(
extern "C" __global__ void __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(4))) es_hoist_wave(Args A) {   // blockDim = 64 WPB
  __shared__ double lk[256], tb[6 * 27];
  __shared__ double ws[WPB][FPW * (WSIZE + PENSZ)];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) lk[i] = A.lktab[i];
  for (int i = threadIdx.x; i < 6 * 27; i += blockDim.x) tb[i] = i < 5 * 27 ? A.tba[i] : 1.0;
T3FILL  __syncthreads();
  // FPW families per wave: lane group h (LPF lanes) hoists the unit's family h in its own slice; `lane` is the lane within
  // the group (`half`: the group, from the pair mode of two)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (LPF - 1);
  const int half = FPW > 1 ? (threadIdx.x & 63) / LPF : 0;
  double* W = ws[wave] + half * (WSIZE + PENSZ);
  double* PEN = W + WSIZE;   // the current (site, family)'s penetrances
  // the de novo transmission rows of this lane's marriage-partial pairs (lane, lane + 64), for every 10-state step
  double tr0[10], tr1[10];
#pragma unroll
  for (int k = 0; k < 10; k++) {
    tr0[k] = A.T10dn[lane * 10 + k];
    tr1[k] = lane + 64 < 100 ? A.T10dn[(lane + 64) * 10 + k] : 0.0;
  }
  const double* t10 = A.T10;
  const double* t10dn = A.T10dn;
  // PM_ES_PROF=1: clock cycles per wave in the pen fill, top rest, leaf prefix, 10-state rest and whole variants
  unsigned long long pc[5] = {0, 0, 0, 0, 0};
#define PCLK(c) if (PROF) { const unsigned long long t1_ = __builtin_readcyclecounter(); pc[c] += t1_ - tq; tq = t1_; }
  const int nItems = min(A.counts[A.list], A.it1);
  if (nItems <= A.it0) return;
  // a task: G consecutive items of the list -- with A.group, the de novo items of one site (list 0: cfgs 0-3, list 1:
  // cfgs 4-6), whose 10-state leaf steps are taken once per (site, family) -- on one family
  const int G = A.group > 1 ? A.group : 1;
  const int nfu = kNUnits;   // family units per task: slots, or units of FPW slots
  const long long units = ((long long)(nItems - A.it0) + G - 1) / G * nfu;
  // the next task's penetrance bytes are loaded while this one is computed (NPF per lane: 10 n <= 64 NPF)
  unsigned pb[NPF > 0 ? NPF : 1];
  long long pf_u = -1;   // the task whose bytes pb holds
  // A task's words are loaded ahead, so no load is waited for when it starts: its G item words two tasks ahead, the
  // sites' reference bytes one task ahead (both uniform); the family unit's slot words are constants of the generated
  // source (kUP0 / kUE / kUSig, per unit and half), so the penetrance-byte prefetch below has no dependent load chain
  int c_item[4], c_ref[4], n1_item[4], n1_ref[4], n2_item[4];
  auto load_items = [&](long long uu, int* it4) {
#pragma unroll
    for (int t = 0; t < 4; t++) it4[t] = -1;
    if (uu >= units) return;
    const int itn = A.it0 + (int)(uu / nfu) * G;
#pragma unroll
    for (int t = 0; t < 4; t++)
      if (t < G && itn + t < nItems) it4[t] = A.items[itn + t];
  };
  auto load_refs = [&](const int* it4, int* r4) {
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int w = __builtin_amdgcn_readfirstlane(it4[t]);
      r4[t] = w >= 0 ? (int)A.ref[w >> 3] : 0;
    }
  };
  auto prefetch = [&](long long uu, int item_w) {   // (item_w: the task's first item word, landed)
    pf_u = -1;
    if (NPF == 0 || uu >= units) return;
    const int uqn = (int)(uu / nfu), kn0 = (int)(uu - (long long)uqn * nfu);
    const int w = __builtin_amdgcn_readfirstlane(item_w);
    if (w < 0) return;
    const int sn = w >> 3;
    const int p0n = kUP0[FPW * kn0 + half];
    const int nn = shape_n(kUSig[kn0]);
    if (10 * nn > LPF * NPF) return;
    const uint8_t* pln = A.pl + (size_t)sn * A.np * 10 + p0n;
#pragma unroll
    for (int r = 0; r < (NPF > 0 ? NPF : 1); r++) {
      const int e = lane + LPF * r, g = e / nn;
      pb[r] = e < 10 * nn ? pln[(size_t)g * A.np + (e - g * nn)] : 0;
    }
    pf_u = uu;
  };
  // XCD-aware unit order: blocks are dealt round-robin over the 8 XCDs, so the units of one round are split into 8
  // contiguous ranges, one per XCD -- a task's family units (one site's penetrance rows) stay in one XCD's L2
  const long long stride = (long long)gridDim.x * WPB;
  const long long u_first = (true && gridDim.x % 8 == 0)
      ? (long long)(blockIdx.x % 8) * (gridDim.x / 8) * WPB + (long long)(blockIdx.x / 8) * WPB + wave
      : (long long)blockIdx.x * WPB + wave;
  load_items(u_first, c_item);
  load_refs(c_item, c_ref);
  load_items(u_first + stride, n1_item);
  load_refs(n1_item, n1_ref);
  load_items(u_first + 2 * stride, n2_item);
  prefetch(u_first, c_item[0]);
  for (long long u = u_first; u < units; u += stride) {
    const int uq = (int)(u / nfu), k0 = (int)(u - (long long)uq * nfu);
    if (u != u_first) {   // rotate: this task's words (landed a task ago), the next task's refs, the task after's items
#pragma unroll
      for (int t = 0; t < 4; t++) { c_item[t] = n1_item[t]; c_ref[t] = n1_ref[t]; n1_item[t] = n2_item[t]; }
      load_refs(n1_item, n1_ref);
      load_items(u + 2 * stride, n2_item);
    }
    // (true: the unit's half -- per lane; both halves share the pair's shape)
    int leaf_site = -1, pen_site = -1;
    unsigned long long tq = PROF ? __builtin_readcyclecounter() : 0;
    for (int t = 0; t < G; t++) {
    const int it = A.it0 + uq * G + t;
    const int item = __builtin_amdgcn_readfirstlane(c_item[t]);
    if (item < 0) break;
    const int site = item >> 3, cfg = item & 7, r = __builtin_amdgcn_readfirstlane(c_ref[t]);
    int a1, a2;
    if (A.vcf) { a1 = r & 15; a2 = r >> 4; }
    else if (cfg == 7) { a1 = A.res[(size_t)site * A.res_words + A.res_a1]; a2 = A.res[(size_t)site * A.res_words + A.res_a2]; }
    else cfg_alleles(cfg, r, &a1, &a2);
    const int g11 = gi(a1, a1), g12 = gi(a1, a2), g22 = gi(a2, a2);
    const uint8_t* pl = A.pl + (size_t)site * A.np * 10;
    const uint8_t* P11 = pl + (size_t)g11 * A.np;
    const uint8_t* P12 = pl + (size_t)g12 * A.np;
    const uint8_t* P22 = pl + (size_t)g22 * A.np;
    const int e = kUE[FPW * k0 + half], q = e / A.T;
    const int sig = kUSig[k0], p0 = kUP0[FPW * k0 + half];
    double* out = A.coef + ((size_t)(it - A.it0) * A.max_ext + q) * A.dcap * A.T + (e - q * A.T);
    const int dn = A.denovo && cfg != 7, top = dn && cfg == 0 && !A.vcf;   // variant: 0 bi-allelic, 1 10-state, 2 top
    if (site != pen_site) {
      if (pf_u == u && t == 0) {   // the prefetched bytes (this task's first item)
        const int nn = shape_n(sig);
#pragma unroll
        for (int r = 0; r < (NPF > 0 ? NPF : 1); r++)
          if (lane + LPF * r < 10 * nn) PEN[lane + LPF * r] = lk[pb[r]];
        wave_sync();
        prefetch(u + stride, n1_item[0]);
      } else {
        switch (sig) {
PENS        }
      }
      pen_site = site;
      PCLK(0);
    }
    if ((G > 1 || PARTS_ONLY) && dn) {
      if (site != leaf_site) {
        leaf_site = site;
        switch (sig) {
PARTS1        }
        PCLK(2);
      }
      if (top) {
        switch (sig) {
PARTS3        }
        PCLK(1);
        continue;
      }
      if (false && t + 3 <= G && it + 2 < nItems) {   // the site's three 10-state items at once (lanes over item x state)
        const int ib = __builtin_amdgcn_readfirstlane(A.items[it + 1]), ic = __builtin_amdgcn_readfirstlane(A.items[it + 2]);
        if ((ib >> 3) == site && (ic >> 3) == site && (ib & 7) != 0 && (ib & 7) != 7 && (ic & 7) != 0 && (ic & 7) != 7) {
          int b1, b2, c1, c2;
          cfg_alleles(ib & 7, r, &b1, &b2);
          cfg_alleles(ic & 7, r, &c1, &c2);
          const int G11 = g11 | gi(b1, b1) << 8 | gi(c1, c1) << 16, G12 = g12 | gi(b1, b2) << 8 | gi(c1, c2) << 16,
                    G22 = g22 | gi(b2, b2) << 8 | gi(c2, c2) << 16;
          const size_t ostr = (size_t)A.max_ext * A.dcap * A.T;
          switch (sig) {
          }
          PCLK(3);
          t += 2;
          continue;
        }
      }
      switch (sig) {
PARTS2      }
      PCLK(3);
      continue;
    }
    leaf_site = -1;   // (the other variants' layouts overlay the leaf prefix's partials)
    switch (sig * 3 + (top ? 2 : dn ? 1 : 0)) {
)";
  auto subst = [](std::string& text, const std::string& token, const std::string& value) {   // every occurrence
    for (size_t at; (at = text.find(token)) != std::string::npos;) text.replace(at, token.size(), value);
  };
  k.replace(k.find("T3FILL"), 6, uses_t3z ? "  for (int i = threadIdx.x; i < 330; i += blockDim.x) {\n    if (i < 320) t3z[i] = kT3z[i];\n"
                                            "    else t3n[i - 320] = kT3n[i - 320];\n  }\n" : "");
  subst(k, "WSIZE", std::to_string(ws));
  subst(k, "PENSZ", std::to_string(pensz));
  subst(k, "NPF", std::to_string(npf));
  subst(k, "LPF", std::to_string(kWl));
  subst(k, "FPW", std::to_string(kFpw));
  {
    std::string cases;
    for (size_t i = 0; i < pens.size(); i++) cases += "        case " + std::to_string(i) + ": " + pens[i] + "(pl, A.np, p0, lk, PEN, lane); break;\n";
    k.replace(k.find("PENS"), 4, cases);
  }
  subst(k, "WPB", std::to_string(wpb));
  k.replace(k.find("PARTS_ONLY"), 10, parts_only ? "true" : "false");
  const std::string call = "(pl, A.np, P11, P12, P22, p0, g11, g12, g22, lk, t10, t10dn, tb, tr0, tr1, W, lane, out, A.T, A.dcap, 0, PEN); break;\n";
  for (int p = 1; p <= 3; p++) {
    std::string cases;
    for (size_t i = 0; 3 * i + p - 1 < parts.size(); i++) cases += "        case " + std::to_string(i) + ": " + parts[3 * i + p - 1] + call;
    const std::string key = "PARTS" + std::to_string(p);
    k.replace(k.find(key), key.size(), cases);
  }
  s += k;
  for (size_t i = 0; i < fns.size(); i++)
    if (!fns[i].empty()) s += "      case " + std::to_string(i) + ": " + fns[i] + call;
  s += "    }\n    PCLK(4);\n    }\n  }\n  if (PROF && lane == 0)\n    for (int c = 0; c < 5; c++) atomicAdd(A.prof + c, pc[c]);\n}\n";
  subst(s, "PROF", opt.prof ? "true" : "false");
  return s;
}

std::mutex g_mu;
std::map<std::pair<int, std::string>, hipModule_t> g_modules;   // (device, source) -> module, for the process

}  // namespace

// Packs one extended family's ES_Peeling schedule for d_es_lk: marriage-partial slots are resolved the
// way the reference's partial map behaves (created by the first type-1 step of a couple, looked up by
// later type-2/3 steps, absent before that).  Returns the workspace doubles the family needs, -1 if it
// cannot be packed (family larger than 255 members).
int pack_steps(const pm_pedigree* ped, int f, int ns, std::vector<int2>& out) {
  const int p0 = ped->fam_start[f], n = ped->fam_start[f + 1] - p0;
  if (n > 255 || !ped->peel_start || !ped->steps) return -1;
  std::vector<std::pair<int, int>> keys;
  auto find = [&](int a, int b) {
    for (size_t i = 0; i < keys.size(); i++) if (keys[i].first == a && keys[i].second == b) return (int)i;
    return -1;
  };
  for (int k = ped->peel_start[f]; k < ped->peel_start[f + 1]; k++) {
    const pm_peel_step& S = ped->steps[k];
    int slot = 255, create = 0, fa2mo = 0;
    if (S.type == 1) {
      int i = find(S.to0, S.to1);
      if (i < 0) { i = (int)keys.size(); keys.push_back({S.to0, S.to1}); create = 1; }
      slot = i;
    } else if (S.type == 2) {
      int a, b;
      if (ped->sex[p0 + S.from0] == FEMALE) { a = S.to0; b = S.from0; fa2mo = 0; } else { a = S.from0; b = S.to0; fa2mo = 1; }
      const int i = find(a, b);
      slot = i < 0 ? 255 : i;
    } else if (S.type == 3) {
      const int i = find(S.from0, S.from1);
      slot = i < 0 ? 255 : i;
    } else return -1;
    if (keys.size() > 254) return -1;
    int2 e;
    e.x = (S.type & 255) | ((S.from0 & 255) << 8) | ((S.from1 & 255) << 16) | ((S.to0 & 255) << 24);
    e.y = (S.to1 & 255) | (slot << 8) | (create << 16) | (fa2mo << 17);
    out.push_back(e);
  }
  if (ped->peel_start[f + 1] == ped->peel_start[f]) return -1;
  return n * ns + (int)keys.size() * ns * ns;
}

std::string generate(int chrom, const std::vector<Family>& fams, const double (*tba)[27], Kernel* out, int denovo) {
  std::map<std::string, int> shape_of;
  for (auto& v : out->shape_ops) v.clear();
  std::vector<std::string> names, bodies, post_names, post_bodies, wave_names, wave_bodies, part_names, pen_names;
  int pensz = 1;
  std::vector<int> shape_ns;   // persons per shape
  auto env_is = [](const char* name, char c) { const char* v = getenv(name); return v && v[0] == c; };
  Opts opt;
  opt.prof = env_is("PM_ES_PROF", '1');
  opt.sp3 = !env_is("PM_ES_SP3", '0');
  opt.t3z = !env_is("PM_ES_T3Z", '0');
  opt.layout = getenv("PM_JIT_LAYOUT") != nullptr;
  opt.steps = getenv("PM_JIT_STEPS") != nullptr;
  bool uses_t3z = false;   // some family of the kernel reads the Mendelian LDS list (emit_type3_dense)
  int ws = 1;
  std::vector<std::pair<int, int>> order;   // (shape, index into fams)
  for (size_t i = 0; i < fams.size(); i++) {
    const std::string key = shape_key(fams[i]);
    auto it = shape_of.find(key);
    int id;
    if (it == shape_of.end()) {
      id = (int)names.size();
      shape_of[key] = id;
      names.push_back("fam" + std::to_string(id));
      double o3[6] = {0, 0, 0, 0, 0, 0};
      if (!denovo) {
        bodies.push_back(gen_family(fams[i], chrom, tba, names.back(), &o3[0]));
        post_names.push_back("post" + std::to_string(id));
        post_bodies.push_back(gen_post_family(fams[i], chrom, tba, post_names.back()));
      } else {   // variants 3 id + {0 bi-allelic, 1 10-state, 2 top}
        pen_names.push_back("wfam" + std::to_string(id) + "_pen");
        shape_ns.push_back(fams[i].n);
        wave_bodies.push_back(gen_pen_fill(fams[i].n, pen_names.back()));
        pensz = std::max(pensz, 10 * fams[i].n);
        for (int v = 0; v < 3; v++) {
          if (denovo == 2 && v > 0) {   // (grouped tasks only: the de novo items go through the parts)
            wave_names.push_back("");
            continue;
          }
          wave_names.push_back("wfam" + std::to_string(id) + "_" + std::to_string(v));
          const WaveFamily A = analyse_wave_family(fams[i], chrom, v == 0 ? 3 : 10, v == 2, wave_names.back(), 0, opt);
          wave_bodies.push_back(emit_wave_family(A, opt, &o3[v], &uses_t3z));
          ws = std::max(ws, A.ws);
        }
        for (int p = 1; p <= 3; p++) {   // the leaf prefix, the 10-state rest, the top rest (grouped tasks)
          part_names.push_back("wfam" + std::to_string(id) + (p == 1 ? "_leaf" : p == 2 ? "_rest" : "_toprest"));
          const WaveFamily A = analyse_wave_family(fams[i], chrom, 10, p == 3, part_names.back(), p == 1 ? 1 : 2, opt);
          wave_bodies.push_back(emit_wave_family(A, opt, &o3[2 + p], &uses_t3z));
          ws = std::max(ws, A.ws);
        }
      }
      for (int v = 0; v < 6; v++) out->shape_ops[v].push_back(o3[v]);
    } else id = it->second;
    order.push_back({id, (int)i});
  }
  std::stable_sort(order.begin(), order.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
  out->slot_e.clear(); out->slot_sig.clear(); out->slot_p0.clear(); out->pair_k.clear();
  for (auto& o : order) {
    out->slot_e.push_back(fams[o.second].e);
    out->slot_sig.push_back(o.first);
    out->slot_p0.push_back(fams[o.second].p0);
  }
  // es_hoist_wave: consecutive slots of one shape form a unit of kFpw (a pair); an odd one out is paired with itself
  // (both halves compute the same family and store the same values to the same coefficients)
  for (size_t i = 0; denovo && i < out->slot_sig.size();) {
    size_t j = i + 1;
    while (j < out->slot_sig.size() && (int)(j - i) < kFpw && out->slot_sig[j] == out->slot_sig[i]) j++;
    for (int f = 0; f < kFpw; f++) out->pair_k.push_back((int)(i + f < j ? i + f : i));
    i = j;
  }
  out->n_shapes = (int)names.size();
  std::string src = kPrologue;
  if (!denovo) {
    for (auto& b : bodies) src += b;
    src += gen_kernel(names);
    src += kPostPrologue;
    for (auto& b : post_bodies) src += b;
    src += gen_post_kernel(post_names);
    out->wave = false;
  } else {
    // waves per block: as many workspace slices as fit the 64 KB of static LDS next to the tables
    const int tables = (256 + 6 * 27) * 8 + (uses_t3z ? (320 + 10) * 4 : 0);
    // (one wave per SIMD: the occupancy comes from blocks per CU, build() asks the runtime for them)
    const int slice = kFpw * (ws + pensz) * 8;   // (a unit's family slices per wave)
    // (at most 4: one wave per SIMD and block; measured on config 4 --denovo, 4 beat 1, 2, 5 and 6 even where those
    // gave more waves per CU -- profiles/r05k_ab_es_wpb.txt)
    const int fit = (64 * 1024 - tables) / slice;
    out->wpb = std::max(0, std::min(4, fit));
    // (wpb 0: a family too large for one slice -- the engine's generic kernel)
    std::string wk = gen_wave_kernel(wave_names, part_names, pen_names, shape_ns, ws, pensz, std::max(1, out->wpb), denovo == 2, uses_t3z, opt);
    const size_t at = wk.find("extern \"C\"");   // device helpers first, then the family functions, then the kernel
    src += wk.substr(0, at);
    {   // the family units' slot words (unit = slot pair; both halves' entries): constants
      const size_t nu = out->pair_k.size() / kFpw;
      const std::string nf = std::to_string(kFpw * nu);
      std::string p0 = "__constant__ int kUP0[" + nf + "] = {", e = "__constant__ int kUE[" + nf + "] = {",
                  sg = "__constant__ int kUSig[" + std::to_string(nu) + "] = {";
      for (size_t u = 0; u < nu; u++) {
        for (int f = 0; f < kFpw; f++) {
          const int k = out->pair_k[kFpw * u + f];
          p0 += std::to_string(out->slot_p0[k]) + ",";
          e += std::to_string(out->slot_e[k]) + ",";
        }
        sg += std::to_string(out->slot_sig[out->pair_k[kFpw * u]]) + ",";
      }
      src += p0 + "};\n" + e + "};\n" + sg + "};\n__device__ constexpr int kNUnits = " + std::to_string(nu) + ";\n";
    }
    if (uses_t3z) {   // the plain Mendelian T(e = i 10 + j, k)'s non-zero terms per child state k, ascending e: e << 2 | code
      auto gi = [](int b1, int b2) { return b1 < b2 ? (b1 - 1) * (10 - b1) / 2 + (b2 - b1) : (b2 - 1) * (10 - b2) / 2 + (b1 - b2); };
      std::vector<double> T(1000, 0.0);
      for (int i = 1; i <= 4; i++)
        for (int j = i; j <= 4; j++)
          for (int k = 1; k <= 4; k++)
            for (int m = k; m <= 4; m++) {
              const int g[4] = {gi(i, k), gi(i, m), gi(j, k), gi(j, m)};
              for (int t = 0; t < 4; t++) T[(gi(i, j) * 10 + gi(k, m)) * 10 + g[t]] += 0.25;
            }
      std::string z = "__shared__ int t3z[320], t3n[10];\n__device__ const int kT3z[320] = {", zn = "__device__ const int kT3n[10] = {";
      for (int k = 0; k < 10; k++) {
        int q = 0;
        for (int e = 0; e < 100; e++) {
          const double t = T[e * 10 + k];
          if (t == 0.0) continue;
          const int code = t == 1.0 ? 0 : t == 0.5 ? 1 : 2;
          if (code == 2 && t != 0.25) { fprintf(stderr, "es_jit: unexpected Mendelian entry\n"); abort(); }
          z += std::to_string(e << 2 | code) + ",";
          q++;
        }
        if (q > 32) { fprintf(stderr, "es_jit: Mendelian list over 32\n"); abort(); }
        for (; q < 32; q++) z += "0,";
        zn += std::to_string([&] { int c = 0; for (int e = 0; e < 100; e++) c += T[e * 10 + k] != 0.0; return c; }()) + ",";
      }
      src += z + "};\n" + zn + "};\n";
    }
    for (auto& b : wave_bodies) src += b;
    src += wk.substr(at);
    out->wave = true;
    out->ws = ws;
  }
  return src;
}

bool compile(const std::string& src, std::vector<char>* code, std::string* err, const std::string& arch) {
  hiprtcProgram prog;
  // the shared device headers (brent_core.h, log_table.h), embedded at build time (Makefile: build/jit_headers.inc)
  const char* hdr[] = {kBrentCoreH, kLogTableH};
  const char* hdr_names[] = {"brent_core.h", "log_table.h"};
  if (hiprtcCreateProgram(&prog, src.c_str(), "es_hoist_jit.hip", 2, hdr, hdr_names) != HIPRTC_SUCCESS) {
    *err = "hiprtcCreateProgram failed";
    return false;
  }
  // -ffp-contract=off: only the explicit fma() of the generated code fuses
  // (the device's own target -- gcnArchName without feature suffixes -- so the module always loads on it)
  const std::string off = "--offload-arch=" + arch;
  // PM_BRENT_UNIFORM: every pm_brent_init of these kernels takes kernel arguments (wave-uniform), which brent_core.h
  // then pins in scalar registers once per item.  (PM_SERIAL_V0: the library built with it -- lib_exp/serial_v0.so --
  // compiles its kernels with brent_core.h's earlier serial path as well.)
#ifdef PM_SERIAL_V0
  const char* opts[] = {off.c_str(), "-O3", "-ffp-contract=off", "-std=c++17", "-DPM_SERIAL_V0=1"};
#else
  const char* opts[] = {off.c_str(), "-O3", "-ffp-contract=off", "-std=c++17", "-DPM_BRENT_UNIFORM=1"};
#endif
  const hiprtcResult rc = hiprtcCompileProgram(prog, (int)(sizeof(opts) / sizeof(opts[0])), opts);
  if (rc != HIPRTC_SUCCESS) {
    size_t ls = 0;
    hiprtcGetProgramLogSize(prog, &ls);
    std::string log(ls + 1, '\0');
    hiprtcGetProgramLog(prog, &log[0]);
    *err = "hipRTC compile of the peeling kernel failed: " + log.substr(0, 2000);
    hiprtcDestroyProgram(&prog);
    return false;
  }
  size_t cs = 0;
  hiprtcGetCodeSize(prog, &cs);
  code->resize(cs);
  hiprtcGetCode(prog, code->data());
  hiprtcDestroyProgram(&prog);
  return true;
}

bool build(int device, int chrom, const std::vector<Family>& fams, const double (*tba)[27], int denovo, Kernel* out,
           std::string* err) {
  const auto t0 = std::chrono::steady_clock::now();
  const std::string src = generate(chrom, fams, tba, out, denovo);
  if (denovo && out->wpb == 0) { *err = "family workspace exceeds a block's LDS"; return false; }
  std::lock_guard<std::mutex> lock(g_mu);
  auto key = std::make_pair(device, src);
  auto it = g_modules.find(key);
  if (it == g_modules.end()) {
    std::vector<char> code;
    std::string arch = "gfx950";
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.gcnArchName[0]) {
      arch = prop.gcnArchName;
      arch = arch.substr(0, arch.find(':'));
    }
    if (!compile(src, &code, err, arch)) return false;
    hipModule_t mod;
    if (hipSetDevice(device) != hipSuccess || hipModuleLoadData(&mod, code.data()) != hipSuccess) {
      *err = "hipModuleLoadData of the peeling kernel failed";
      return false;
    }
    it = g_modules.emplace(key, mod).first;
  }
  const bool ok = denovo ? hipModuleGetFunction(&out->fn, it->second, "es_hoist_wave") == hipSuccess
                         : hipModuleGetFunction(&out->fn, it->second, "es_hoist_jit") == hipSuccess &&
                               hipModuleGetFunction(&out->fn_post, it->second, "es_post_jit") == hipSuccess;
  if (!ok) {
    *err = "hipModuleGetFunction of the generated kernels failed";
    return false;
  }
  if (denovo) {   // resident blocks per CU (VGPRs and LDS): the launch's grid
    int nb = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, out->fn, 64 * out->wpb, 0) != hipSuccess) nb = 0;
    out->blocks_per_cu = nb;
    if (getenv("PM_JIT_LAYOUT")) fprintf(stderr, "es_hoist_wave: wpb %d ws %d blocks/CU %d\n", out->wpb, out->ws, nb);
  }
  out->compile_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return true;
}

// ---------------------------------------------------------------------------------------------------------------
// ep_brent_jit: the fused hoisting + Brent kernel (es_jit.h FusedKernel).  Layout: families sorted by (degree
// descending, shape), dealt row-major onto rows of `lanes` cells; each row's register tile holds its largest degree
// + 1 coefficients.  The lane count is chosen by a cost model of one item: hoisting = the generated peels' operations
// of every shape present in a row (a row's lanes run the shapes it holds one after the other), evaluations = about
// 30 Brent evaluations x 2 (D_row + 1) Horner operations per row; a lane's degrees summed stay <= 64 (g^D >= 1e-256
// at Brent's start b = 0.9999) and the tiles <= 64 doubles.
std::string generate_fused(int chrom, const std::vector<Family>& fams, const double (*tba)[27], FusedKernel* out) {
  const int n = (int)fams.size();
  out->lane_tab.clear(); out->row_deg.clear(); out->rows = out->lanes = out->n_shapes = 0; out->item_ops = 0;
  if (n == 0) return "";
  std::map<std::string, int> shape_of;
  std::vector<std::string> bodies;
  std::vector<int> sdeg;
  std::vector<double> sops;
  std::vector<int> sig(n);
  for (int i = 0; i < n; i++) {
    const std::string key = shape_key(fams[i]);
    auto it = shape_of.find(key);
    if (it == shape_of.end()) {
      const int id = (int)bodies.size();
      shape_of[key] = id;
      double o = 0;
      int d = 0;
      bodies.push_back(gen_family(fams[i], chrom, tba, "ffam" + std::to_string(id), &o, true, &d));
      sdeg.push_back(d);
      sops.push_back(o);
      sig[i] = id;
    } else sig[i] = it->second;
  }
  const int ns = (int)bodies.size();
  if (ns > 127) return "";
  std::vector<int> order(n);
  for (int i = 0; i < n; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    return sdeg[sig[a]] != sdeg[sig[b]] ? sdeg[sig[a]] > sdeg[sig[b]] : sig[a] < sig[b];
  });
  // Two layouts: one item per wave (rows of up to 64 cells), or two (pair: each half-wave, 32 lanes, runs its own item
  // on rows of up to 32 cells -- the evaluation's fixed part (division, power, reduction, log10, Brent's update) is then
  // shared by two items, at the price of twice the rows and of the longer of the two Brent runs).  Per-item cost model:
  // hoisting + kEvals x (2 (D_row + 1) per row + the fixed part), the pair layout's halved.
  const int kRowsMax = 8, kTile = 64, kEvals = 30;
  const double kFixed1 = 150, kFixed2 = 230, kImb = 1.1;
  const char* epair = getenv("PM_FUSED_PAIR");   // (0 / 1: force one layout)
  double best = -1;
  int best_nl = 0;
  bool pair = false;
  for (int pm = 0; pm < 2; pm++) {
    if (epair && atoi(epair) != pm) continue;
    const int lmax = pm ? 32 : 64;
    for (int nl = (n + kRowsMax - 1) / kRowsMax; nl <= lmax; nl++) {
      if (nl <= 0) continue;
      const int rows = (n + nl - 1) / nl;
      double hoist = 0, eval = pm ? kFixed2 : kFixed1;
      int tile = 0;
      std::vector<int> lane_deg(nl, 0);
      for (int r = 0; r < rows; r++) {
        std::vector<char> seen(ns, 0);
        int dmax = 0;
        for (int k = r * nl; k < std::min(n, (r + 1) * nl); k++) {
          const int sg = sig[order[k]];
          if (!seen[sg]) { seen[sg] = 1; hoist += sops[sg]; }
          dmax = std::max(dmax, sdeg[sg]);
          lane_deg[k - r * nl] += sdeg[sg];
        }
        tile += dmax + 1;
        eval += 2.0 * (dmax + 1);
      }
      if (tile > kTile || *std::max_element(lane_deg.begin(), lane_deg.end()) > 64) continue;
      const double cost = pm ? (hoist + kImb * kEvals * eval) / 2 : hoist + kEvals * eval;
      if (best < 0 || cost < best) { best = cost; best_nl = nl; pair = pm; }
    }
  }
  if (best_nl == 0) return "";
  const int nl = best_nl, rows = (n + nl - 1) / nl;
  out->lanes = nl; out->rows = rows; out->n_shapes = ns; out->pair = pair;
  out->lane_tab.assign((size_t)rows * 64 + 64, -1);
  for (int l = 0; l < 64; l++) out->lane_tab[(size_t)rows * 64 + l] = 0;
  std::vector<std::vector<int>> row_shapes(rows);
  for (int r = 0; r < rows; r++) {
    int dmax = 0;
    for (int k = r * nl; k < std::min(n, (r + 1) * nl); k++) {
      const Family& F = fams[order[k]];
      const int sg = sig[order[k]], l = k - r * nl;
      out->lane_tab[(size_t)r * 64 + l] = F.p0 | (sg << 24);
      out->lane_tab[(size_t)rows * 64 + l] += sdeg[sg];
      if (std::find(row_shapes[r].begin(), row_shapes[r].end(), sg) == row_shapes[r].end()) row_shapes[r].push_back(sg);
      dmax = std::max(dmax, sdeg[sg]);
    }
    out->row_deg.push_back(dmax);
  }
  if (pair)   // (both halves hoist the same families for their own items)
    for (int r = 0; r <= rows; r++)
      for (int l = 32; l < 64; l++) out->lane_tab[(size_t)r * 64 + l] = out->lane_tab[(size_t)r * 64 + l - 32];
  for (int i = 0; i < n; i++) out->item_ops += sops[sig[i]];
  if (getenv("PM_JIT_LAYOUT")) {
    fprintf(stderr, "ep_brent_jit: %d families, %d shapes, %d rows x %d lanes%s, tiles", n, ns, rows, nl, pair ? " (two items per wave)" : "");
    for (int r = 0; r < rows; r++) fprintf(stderr, " %d(%zu)", out->row_deg[r], row_shapes[r].size());
    fprintf(stderr, ", cost %.0f\n", best);
  }
  std::string src = kPrologue;
  src += "#include \"brent_core.h\"\n";
  src += R"(
struct FusedArgs {
  const int* items; int* counts; const uint8_t* ref; const int* res; const uint8_t* pl; const double* lktab; const int* lane_tab;
  double* raw; double* minv; int* evals; unsigned long long* eval_total;
  double precision;
  int list, it0, it1, np, vcf, res_words, res_a1, res_a2, itmax, pad;
};
)";
  for (auto& b : bodies) src += b;
  src += "extern \"C\" __global__ void __launch_bounds__(64) ep_brent_jit(FusedArgs A) {\n";
  src += R"(  __shared__ double lk[256];
  for (int i = threadIdx.x; i < 256; i += 64) lk[i] = A.lktab[i];
  __syncthreads();
  const int lane = threadIdx.x;
  const int nItems = min(A.counts[A.list], A.it1);
  // XCD-aware item order (blocks go round-robin to the 8 XCDs): consecutive items -- one site's configurations, one
  // PL block -- on blocks of one XCD
  const int vb = (gridDim.x % 8 == 0) ? (blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8 : blockIdx.x;
)";
  src += "  int ltab[" + std::to_string(rows) + "];\n";
  src += "#pragma unroll\n  for (int r = 0; r < " + std::to_string(rows) + "; r++) ltab[r] = A.lane_tab[r * 64 + lane];\n";
  src += "  const int edl = A.lane_tab[" + std::to_string(rows * 64) + " + lane];   // g^edl: the lane's degrees summed\n";
  if (!pair)
    src += R"(  unsigned long long ev_acc = 0;
  for (int it = A.it0 + vb; it < nItems; it += gridDim.x) {
    const int item = A.items[it];
)";
  else   // half-wave h takes item it0 + 2 t + h (a missing second item: the first one's data, nothing written)
    src += R"(  unsigned long long ev_acc = 0;
  const int half = lane >> 5;
  for (int t2 = vb; A.it0 + 2 * t2 < nItems; t2 += gridDim.x) {
    const int it = A.it0 + 2 * t2 + half;
    const bool valid = it < nItems;
    const int item = A.items[valid ? it : it - 1];
)";
  src += R"(

    const int site = item >> 3, cfg = item & 7, rb = A.ref[site];
    int a1, a2;
    if (A.vcf) { a1 = rb & 15; a2 = rb >> 4; }
    else if (cfg == 7) { a1 = A.res[(size_t)site * A.res_words + A.res_a1]; a2 = A.res[(size_t)site * A.res_words + A.res_a2]; }
    else cfg_alleles(cfg, rb, &a1, &a2);
    const uint8_t* pls = A.pl + (size_t)site * A.np * 10;
    const uint8_t* P11 = pls + (size_t)gi(a1, a1) * A.np;
    const uint8_t* P12 = pls + (size_t)gi(a1, a2) * A.np;
    const uint8_t* P22 = pls + (size_t)gi(a2, a2) * A.np;
)";
  for (int r = 0; r < rows; r++) {
    const int D = out->row_deg[r];
    const std::string c = "c" + std::to_string(r), R = std::to_string(r);
    src += "    double " + c + "[" + std::to_string(D + 1) + "];\n";
    src += "    if (ltab[" + R + "] < 0) {   // no family: the unit polynomial\n      " + c + "[0] = 1.0;\n";
    for (int a = 1; a <= D; a++) src += "      " + c + "[" + std::to_string(a) + "] = 0.0;\n";
    src += "    } else {\n      const int p0 = ltab[" + R + "] & 0xFFFFFF, sg = ltab[" + R + "] >> 24;\n";
    for (size_t k = 0; k < row_shapes[r].size(); k++) {
      const int sg = row_shapes[r][k];
      src += std::string(k == 0 ? "      " : " else ") +
             (k + 1 < row_shapes[r].size() ? "if (sg == " + std::to_string(sg) + ") " : "") + "{\n";
      src += "        ffam" + std::to_string(sg) + "(P11, P12, P22, p0, lk, " + c + ");\n";
      for (int a = sdeg[sg] + 1; a <= D; a++) src += "        " + c + "[" + std::to_string(a) + "] = 0.0;\n";
      src += "      }";
    }
    src += "\n    }\n";
  }
  src += R"(    PmBrent B;
    pm_brent_init(B, A.precision, A.itmax);
)";
  if (pair) src += "    bool done = !valid;\n";
  src += R"(    for (;;) {
      // every family L = g^D sum_a c_a t^a, t = f / g (non-negative terms: no cancellation), FMA Horner over the row's
      // tile (zeros above a family's own degree leave the sum's bits unchanged); the values split into mantissa and
      // exponent, multiplied in one chain with g^edl, one renormalisation -- as k_brent's EP evaluation
      const double g = 1.0 - B.x;
      const double t = pos_div(B.x, g);
)";
  {   // g^edl: the layout's distinct lane degree sums are known here -- shared squarings, one power per value, a select
    std::vector<int> vals;
    for (int l = 0; l < 64; l++) {
      const int v = out->lane_tab[(size_t)rows * 64 + l];
      if (v > 0 && std::find(vals.begin(), vals.end(), v) == vals.end()) vals.push_back(v);
    }
    std::sort(vals.begin(), vals.end());
    int top = 0;
    for (int v : vals) top = std::max(top, v);
    int nb = 0;
    while ((1 << (nb + 1)) <= top) nb++;   // the highest bit of any value
    src += "      double q0 = g;\n";
    for (int b = 1; b <= nb; b++) src += "      const double q" + std::to_string(b) + " = q" + std::to_string(b - 1) + " * q" + std::to_string(b - 1) + ";\n";
    src += "      double pw = 1.0;\n";
    for (size_t k = 0; k < vals.size(); k++) {
      std::string prod;
      for (int b = 0; b <= nb; b++)   // (ascending bits: the order of the former square-and-multiply loop)
        if ((vals[k] >> b) & 1) prod = prod.empty() ? "q" + std::to_string(b) : "(" + prod + ") * q" + std::to_string(b);
      src += "      if (edl == " + std::to_string(vals[k]) + ") pw = " + prod + ";\n";
    }
  }
  src += "      int e = 0;\n";
  for (int r = 0; r < rows; r++) {
    const int D = out->row_deg[r];
    const std::string c = "c" + std::to_string(r), R = std::to_string(r);
    src += "      double m" + R + ";\n      {\n        double acc = " + c + "[" + std::to_string(D) + "];\n";
    for (int a = D - 1; a >= 0; a--) src += "        acc = fma(acc, t, " + c + "[" + std::to_string(a) + "]);\n";
    src += "        int e1;\n        m" + R + " = frexp(acc, &e1);\n        e += e1;\n      }\n";
  }
  src += "      double m = m0";
  for (int r = 1; r < rows; r++) src += " * m" + std::to_string(r);
  src += R"(;
      int e2;
      m = frexp(m * pw, &e2);
      e += e2;
)";
  if (!pair)
    src += R"(      wave_prod(m, e);
      if (!pm_brent_feed(B, -log10_mant_u(m, e))) break;
    }
    if (lane == 0) {
)";
  else   // (a half whose Brent has ended keeps its state; the wave goes on until both have)
    src += R"(      wave_prod_pair(m, e);
      const double fx = -log10_mant_pair(m, e);
      if (!done && !pm_brent_feed(B, fx)) done = true;
      if (__ballot(!done) == 0) break;
    }
    if ((lane & 31) == 0 && valid) {
)";
  src += R"(      A.raw[(size_t)site * 8 + cfg] = -B.fmin;
      A.minv[(size_t)site * 8 + cfg] = B.mn;
      A.evals[(size_t)site * 8 + cfg] = B.nev;
      ev_acc += B.nev - 2;   // objective evaluations computed (f(a), f(c) counted only)
      if (!B.ok) { atomicExch(&A.counts[5], 1); atomicMin(&A.counts[6], site); }   // (the reference stops at the first)
    }
  }
  if ((lane & 31) == 0 && ev_acc) atomicAdd(A.eval_total, ev_acc);
}
)";
  return src;
}

bool build_fused(int device, int chrom, const std::vector<Family>& fams, const double (*tba)[27], FusedKernel* out,
                 std::string* err) {
  const auto t0 = std::chrono::steady_clock::now();
  const std::string src = generate_fused(chrom, fams, tba, out);
  if (src.empty()) { *err = "the families do not fit the fused kernel's register tiles"; return false; }
  std::lock_guard<std::mutex> lock(g_mu);
  auto key = std::make_pair(device, src);
  auto it = g_modules.find(key);
  if (it == g_modules.end()) {
    std::vector<char> code;
    std::string arch = "gfx950";
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.gcnArchName[0]) {
      arch = prop.gcnArchName;
      arch = arch.substr(0, arch.find(':'));
    }
    if (!compile(src, &code, err, arch)) return false;
    hipModule_t mod;
    if (hipSetDevice(device) != hipSuccess || hipModuleLoadData(&mod, code.data()) != hipSuccess) {
      *err = "hipModuleLoadData of the fused Brent kernel failed";
      return false;
    }
    it = g_modules.emplace(key, mod).first;
  }
  if (hipModuleGetFunction(&out->fn, it->second, "ep_brent_jit") != hipSuccess) {
    *err = "hipModuleGetFunction(ep_brent_jit) failed";
    return false;
  }
  int nb = 0;
  if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, out->fn, 64, 0) != hipSuccess) nb = 0;
  out->blocks_per_cu = nb;
  if (getenv("PM_JIT_LAYOUT")) fprintf(stderr, "ep_brent_jit: blocks/CU %d\n", nb);
  out->compile_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return true;
}

}  // namespace pmjit
