// PyTorch bindings for the spark_gp_amd CDNA4 HIP kernels.

#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>

#include <climits>
#include <initializer_list>
#include <tuple>
#include <vector>

#include "kernel_geom.h"
#include "launchers.h"

namespace {

void check_hip(hipError_t err, const char* what) {
  TORCH_CHECK(err == hipSuccess, what, ": ", hipGetErrorString(err));
}

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// ---- argument validation --------------------------------------------------
// Every binding checks dtype, rank and shape of each argument first (tensor
// metadata only, so these also work on CPU tensors) and the devices last,
// before anything is allocated or launched.

constexpr int64_t ANY = -1;   // a free size in check_arg
constexpr auto F32 = torch::kFloat32, F64 = torch::kFloat64;
constexpr auto BF16 = torch::kBFloat16, I32 = torch::kInt32;

void check_dtype(const torch::Tensor& t, const char* name,
                 torch::ScalarType dtype, bool in_place) {
  TORCH_CHECK(t.scalar_type() == dtype, name, " must be ", dtype, ", got ",
              t.scalar_type());
  // a kernel cannot write through a contiguous copy
  TORCH_CHECK(!in_place || t.is_contiguous(), name, " must be contiguous");
}

void check_arg(const torch::Tensor& t, const char* name,
               torch::ScalarType dtype, std::initializer_list<int64_t> sizes,
               bool in_place = false) {
  check_dtype(t, name, dtype, in_place);
  bool ok = t.dim() == (int64_t)sizes.size();
  for (size_t i = 0; ok && i < sizes.size(); ++i)
    ok = sizes.begin()[i] == ANY || t.size(i) == sizes.begin()[i];
  TORCH_CHECK(ok, name, " must have shape ", c10::IntArrayRef(sizes),
              " (-1: any), got ", t.sizes());
}

// a vector of n elements of any rank ([n], [n, 1], ...)
void check_vec(const torch::Tensor& t, const char* name,
               torch::ScalarType dtype, int64_t n, bool in_place = false) {
  check_dtype(t, name, dtype, in_place);
  TORCH_CHECK(t.numel() == n, name, " must have ", n, " elements, got ",
              t.numel());
}

struct Arg {
  const torch::Tensor* t;   // null: an absent optional argument
  const char* name;
};

// Every tensor is on a GPU, and all on the same one.
void check_same_gpu(std::initializer_list<Arg> args) {
  const Arg* first = nullptr;
  for (const Arg& a : args) {
    if (!a.t) continue;
    TORCH_CHECK(a.t->is_cuda(), a.name, " must be on the GPU, got ",
                a.t->device());
    if (!first) first = &a;
    TORCH_CHECK(a.t->device() == first->t->device(), a.name, " is on ",
                a.t->device(), " but ", first->name, " is on ",
                first->t->device());
  }
}

void* ptr_or_null(const torch::Tensor& t) {
  return t.defined() ? t.data_ptr() : nullptr;
}

// kernels take dense inputs: replace each by its contiguous form
void make_contiguous(std::initializer_list<torch::Tensor*> ts) {
  for (torch::Tensor* t : ts) *t = t->contiguous();
}

// the covariance family code of an entry point (kernel_geom.h)
void check_family(int64_t family) {
  TORCH_CHECK(geom_family_ok(family), "family must be 0 (RBF), 1 (Matern "
              "3/2) or 2 (Matern 5/2), got ", family);
}

torch::TensorOptions like(const torch::Tensor& t, torch::ScalarType dtype) {
  return torch::TensorOptions().dtype(dtype).device(t.device());
}

}  // namespace

// Returns (nll[E] f64, sumW0[E] f64, trG[E] f64, contr[E,d] f64, bad[E] i32)
std::vector<torch::Tensor> fused_expert_nll_impl(torch::Tensor X,
                                                 torch::Tensor y,
                                                 torch::Tensor scale,
                                                 double amp, double noise,
                                                 bool profile,
                                                 int64_t family) {
  check_family(family);
  check_arg(X, "X", F32, {ANY, ANY, ANY});
  const int E = X.size(0), k = X.size(1), d = X.size(2);
  check_arg(y, "y", F32, {E, k});
  check_vec(scale, "scale", F32, d);
  TORCH_CHECK(k <= 128 && d <= 128, "X must be [E, k, d] with k<=128, "
              "d<=128 for fused_expert_nll, got ", X.sizes());
  check_same_gpu({{&X, "X"}, {&y, "y"}, {&scale, "scale"}});
  make_contiguous({&X, &y, &scale});
  auto nll = torch::empty({E}, like(X, F64));
  auto sumW0 = torch::empty_like(nll), trG = torch::empty_like(nll);
  auto contr = torch::empty({E, d}, like(X, F64));
  auto bad = torch::empty({E}, like(X, I32));
  torch::Tensor clk;
  unsigned long long* clk_ptr = nullptr;
  if (profile) {
    clk = torch::zeros({E, 20}, like(X, torch::kInt64));
    clk_ptr = (unsigned long long*)clk.data_ptr<int64_t>();
  }
  check_hip(launch_fused_expert_nll(
                X.data_ptr<float>(), y.data_ptr<float>(),
                scale.data_ptr<float>(), (float)amp, (float)noise, E, k, d,
                nll.data_ptr<double>(), sumW0.data_ptr<double>(),
                trG.data_ptr<double>(), contr.data_ptr<double>(),
                bad.data_ptr<int>(), clk_ptr, (int)family, current_stream()),
            "fused_expert_nll");
  if (profile) return {nll, sumW0, trG, contr, bad, clk};
  return {nll, sumW0, trG, contr, bad};
}

std::vector<torch::Tensor> fused_expert_nll(torch::Tensor X, torch::Tensor y,
                                            torch::Tensor scale, double amp,
                                            double noise, int64_t family) {
  return fused_expert_nll_impl(X, y, scale, amp, noise, false, family);
}

bool fused_expert_nll_supported(int64_t k, int64_t d) {
  if (k > 128 || d > 128 || k < 1) return false;
  return nll_lds_bytes((int)k, (int)d) <= GEOM_LDS_MAX;
}

// Workgroups of the family's fused_expert_nll kernel the HIP runtime reports resident per
// CU (hipOccupancyMaxActiveBlocksPerMultiprocessor) at the launch's real
// block size and dynamic LDS, on the current device.
int64_t fused_expert_nll_occupancy(int64_t k, int64_t d, int64_t family) {
  check_family(family);
  TORCH_CHECK(k >= 1 && k <= 128, "k must be in [1, 128], got ", k);
  TORCH_CHECK(d >= 1 && d <= 128, "d must be in [1, 128], got ", d);
  int wgs = 0;
  check_hip(fused_expert_nll_resident_wgs((int)k, (int)d, (int)family, &wgs),
            "fused_expert_nll_occupancy");
  return wgs;
}

// The elementwise tile (q by differences, then the family's Kb) in both of
// its uses.  want_cm: write the
// [c, m] copies (hi, and lo with hilo); want_t: write the transposed hi/lo
// pair; y/Ky (both or neither): also accumulate Ky += K^T y from the fp32
// register values.  Returns the tensors written, in the order
// (out, lo, outT, loT).
static std::vector<torch::Tensor> cross_tile(
    const char* what, torch::Tensor X, torch::Tensor A, torch::Tensor s2v,
    double amp, bool bf16_out, bool want_cm, bool hilo, bool want_t,
    torch::Tensor* y, const torch::Tensor* Ky, int64_t family) {
  check_family(family);
  check_arg(X, "X", F32, {ANY, ANY});
  const int c = X.size(0), d = X.size(1);
  check_arg(A, "A", F32, {ANY, d});
  const int m = A.size(0);
  check_vec(s2v, "s2v", F32, d);
  if (y) {
    check_vec(*y, "y", F32, c);
    check_vec(*Ky, "Ky", F64, m, true);
  }
  check_same_gpu({{&X, "X"}, {&A, "A"}, {&s2v, "s2v"}, {y, "y"}, {Ky, "Ky"}});
  make_contiguous({&X, &A, &s2v});
  if (y) make_contiguous({y});
  auto opts = like(X, bf16_out ? BF16 : F32);
  torch::Tensor out, lo, outT, loT;
  if (want_cm) out = torch::empty({c, m}, opts);
  if (want_cm && hilo) lo = torch::empty({c, m}, opts);
  if (want_t) {
    outT = torch::empty({m, c}, opts);
    loT = torch::empty({m, c}, opts);
  }
  check_hip(launch_cross_kernel_tile(
                X.data_ptr<float>(), A.data_ptr<float>(),
                s2v.data_ptr<float>(), (float)amp, c, m, d, ptr_or_null(out),
                ptr_or_null(lo), ptr_or_null(outT), ptr_or_null(loT),
                bf16_out ? 1 : 0,
                y ? y->data_ptr<float>() : nullptr,
                y ? Ky->data_ptr<double>() : nullptr, (int)family,
                current_stream()),
            what);
  std::vector<torch::Tensor> res;
  for (const auto& t : {out, lo, outT, loT})
    if (t.defined()) res.push_back(t);
  return res;
}

std::vector<torch::Tensor> cross_kernel_tile(torch::Tensor X, torch::Tensor A,
                                             torch::Tensor s2v, double amp,
                                             bool bf16_out, bool hilo,
                                             bool want_t, int64_t family) {
  TORCH_CHECK(!hilo || bf16_out, "hilo requires bf16 output");
  TORCH_CHECK(!want_t || hilo, "transposed outputs require hilo bf16 mode");
  return cross_tile("cross_kernel_tile", X, A, s2v, amp, bf16_out, true, hilo,
                    want_t, nullptr, nullptr, family);
}

// PPA fast path: transposed hi/lo tiles ONLY (no [c, m] copies written)
// plus the fused column-sum Ky += K^T y accumulated from the fp32
// register values (replaces the colsum_gemv re-read pass).
std::vector<torch::Tensor> cross_kernel_tile_ppa(torch::Tensor X,
                                                 torch::Tensor A,
                                                 torch::Tensor s2v,
                                                 double amp, torch::Tensor y,
                                                 torch::Tensor Ky,
                                                 int64_t family) {
  return cross_tile("cross_kernel_tile_ppa", X, A, s2v, amp, true, false,
                    true, true, &y, &Ky, family);
}

// Shapes of the pre-scaled PPA inputs shared by cross_mfma_ppa and
// ppa_fused_acc: Xs [c, d], As [m, d], their squared norms, y and Ky.
static void check_ppa_inputs(const torch::Tensor& Xs, const torch::Tensor& As,
                             const torch::Tensor& nx, const torch::Tensor& na,
                             const torch::Tensor& y, const torch::Tensor& Ky) {
  check_arg(Xs, "Xs", F32, {ANY, ANY});
  check_arg(As, "As", F32, {ANY, Xs.size(1)});
  check_vec(nx, "nx", F32, Xs.size(0));
  check_vec(na, "na", F32, As.size(0));
  check_vec(y, "y", F32, Xs.size(0));
  check_vec(Ky, "Ky", F64, As.size(0), true);
}

// MFMA PPA tile: pre-scaled inputs + norms; K1's sqdist-via-GEMM plan.
std::vector<torch::Tensor> cross_mfma_ppa(torch::Tensor Xs, torch::Tensor As,
                                          torch::Tensor nx, torch::Tensor na,
                                          double amp, torch::Tensor y,
                                          torch::Tensor Ky, int64_t family) {
  check_family(family);
  check_ppa_inputs(Xs, As, nx, na, y, Ky);
  check_same_gpu({{&Xs, "Xs"}, {&As, "As"}, {&nx, "nx"}, {&na, "na"},
                  {&y, "y"}, {&Ky, "Ky"}});
  const int c = Xs.size(0), m = As.size(0), d = Xs.size(1);
  make_contiguous({&Xs, &As, &nx, &na, &y});
  auto outT = torch::empty({m, c}, like(Xs, BF16));
  auto loT = torch::empty_like(outT);
  check_hip(launch_cross_mfma(Xs.data_ptr<float>(), As.data_ptr<float>(),
                              nx.data_ptr<float>(), na.data_ptr<float>(),
                              (float)amp, c, m, d, outT.data_ptr(),
                              loT.data_ptr(), y.data_ptr<float>(),
                              Ky.data_ptr<double>(), (int)family,
                              current_stream()),
            "cross_mfma_ppa");
  return {outT, loT};
}

// Checked, contiguous operands of the two SYRK wrappers: KcT/KlT are the
// TRANSPOSED kernel blocks [m, c] (k along the contiguous axis; see
// syrk_bf16_kernel; the second is undefined without KlT), KK [m, m] is
// accumulated in place.  `more`: the wrapper's further tensor, if any.
static std::pair<torch::Tensor, torch::Tensor> syrk_operands(
    const torch::Tensor& KcT, const c10::optional<torch::Tensor>& KlT,
    const torch::Tensor& KK, Arg more = {nullptr, ""}) {
  check_arg(KcT, "KcT", BF16, {ANY, ANY});
  const int64_t m = KcT.size(0), c = KcT.size(1);
  if (KlT.has_value()) check_arg(*KlT, "KlT", BF16, {m, c});
  check_arg(KK, "KK", F32, {m, m}, true);   // m = KcT.size(0)
  check_same_gpu({{&KcT, "KcT"}, {KlT.has_value() ? &*KlT : nullptr, "KlT"},
                  {&KK, "KK"}, more});
  return {KcT.contiguous(),
          KlT.has_value() ? KlT->contiguous() : torch::Tensor()};
}

void syrk_bf16_acc(torch::Tensor KcT, c10::optional<torch::Tensor> KlT,
                   torch::Tensor KK, int64_t split_k) {
  TORCH_CHECK(split_k >= 1 && split_k <= 65535,   // becomes gridDim.y
              "split_k out of range [1, 65535]: ", split_k);
  auto [Kc, Kl] = syrk_operands(KcT, KlT, KK);
  const int m = Kc.size(0), c = Kc.size(1);
  check_hip(launch_syrk_bf16(Kc.data_ptr(), ptr_or_null(Kl), c, m, c,
                             (int)split_k, KK.data_ptr<float>(),
                             current_stream()),
            "syrk_bf16");
}

// k-synchronized SYRK (large m): tiles [nb, 2] int32 (ti, tj; -1 pads),
// one block per tile, accumulators held across all k; see cross_syrk.hip.
// Only the shape of `tiles` is checked: reading its contents would
// synchronise with the device.  They stay trusted — ppa_plan's
// syrk_sync_tile_lists is the only producer.
void syrk_bf16_sync_acc(torch::Tensor KcT, c10::optional<torch::Tensor> KlT,
                        torch::Tensor KK, torch::Tensor tiles,
                        int64_t kpb, int64_t nactive) {
  check_arg(tiles, "tiles", I32, {ANY, 2}, true);
  TORCH_CHECK(kpb >= 1 && kpb <= INT_MAX, "kpb must be >= 1, got ", kpb);
  TORCH_CHECK(nactive >= 0 && nactive <= tiles.size(0),
              "nactive out of range [0, tiles.size(0) = ", tiles.size(0),
              "]: ", nactive);
  auto [Kc, Kl] = syrk_operands(KcT, KlT, KK, {&tiles, "tiles"});
  const int m = Kc.size(0), c = Kc.size(1);
  const int kblocks = (c + SY_BK - 1) / SY_BK;
  const int nphases = (kblocks + (int)kpb - 1) / (int)kpb;
  auto ctr = torch::zeros({nphases}, like(KK, I32));
  check_hip(launch_syrk_bf16_sync(
                Kc.data_ptr(), ptr_or_null(Kl), c, m, c, tiles.data_ptr<int>(),
                (int)tiles.size(0), (int)kpb, ctr.data_ptr<int>(),
                (int)nactive, KK.data_ptr<float>(), current_stream()),
            "syrk_bf16_sync");
}

// Fused PPA accumulation: KK += K^T K (hi/lo bf16 products) and
// Ky += K^T y with the K_nm windows generated inside the SYRK blocks from
// the pre-scaled inputs (see syrk_fused_gen_kernel) — no K_nm in memory.
bool ppa_fused_supported(int64_t m, int64_t d) {
  if (m < 1 || d < 1 || d > SF_DMAX) return false;
  const int64_t ntile = (m + SY_CT - 1) / SY_CT;
  return ntile * (ntile + 1) / 2 <= SY_SPLITK_MAX_TILES;
}

//
// gen selects how the blocks form x'.a': "f16" from two-term f16 images of
// the coordinates on the 16-bit matrix pipe, "f32" on the fp32 one, "auto"
// f16 when the coordinates are inside its range.  The f16 images overflow at
// 65504, so "f16" and "auto" need a bound on |Xs| and |As|: absmax when the
// caller has one (hip_backend takes it once per accumulation), else the
// binding reduces both tensors itself, which synchronises with the device.
// "auto" falls back to f32 at or above SF_F16_ABS_LIMIT, "f16" is refused
// there; a NaN bound counts as out of range.
//
// partials: scratch for the k-slices' tiles (ppa_fused_partials_numel
// elements or more, contents irrelevant), so a caller with many chunks
// allocates it once; allocated here when absent.
void ppa_fused_acc(torch::Tensor Xs, torch::Tensor As, torch::Tensor nx,
                   torch::Tensor na, double amp, torch::Tensor y,
                   torch::Tensor Ky, torch::Tensor KK, int64_t split_k,
                   int64_t family, const std::string& gen,
                   c10::optional<double> absmax,
                   c10::optional<torch::Tensor> partials) {
  check_family(family);
  TORCH_CHECK(gen == "auto" || gen == "f16" || gen == "f32",
              "gen must be \"auto\", \"f16\" or \"f32\", got \"", gen, "\"");
  check_ppa_inputs(Xs, As, nx, na, y, Ky);
  const int c = Xs.size(0), m = As.size(0), d = Xs.size(1);
  TORCH_CHECK(ppa_fused_supported(m, d), "As: unsupported (m, d) for "
              "ppa_fused_acc; query ppa_fused_supported");
  check_arg(KK, "KK", F32, {m, m}, true);
  TORCH_CHECK(split_k >= 1 && split_k <= 65535,
              "split_k out of range [1, 65535]: ", split_k);
  const int64_t part_floats = (int64_t)sf_partial_floats(c, m, split_k);
  if (partials.has_value()) {
    check_dtype(*partials, "partials", F32, true);
    TORCH_CHECK(partials->numel() >= part_floats, "partials must have at "
                "least ", part_floats, " elements for this (c, m, split_k), "
                "got ", partials->numel());
  }
  check_same_gpu({{&Xs, "Xs"}, {&As, "As"}, {&nx, "nx"}, {&na, "na"},
                  {&y, "y"}, {&Ky, "Ky"}, {&KK, "KK"},
                  {partials.has_value() ? &*partials : nullptr, "partials"}});
  if (c == 0) return;
  torch::Tensor part = partials.has_value()
                           ? *partials
                           : torch::empty({part_floats}, like(KK, F32));
  bool gen_f16 = false;
  if (gen != "f32") {
    double bound;
    if (absmax.has_value()) {
      bound = *absmax;
    } else {
      const auto [xlo, xhi] = at::aminmax(Xs);
      const auto [alo, ahi] = at::aminmax(As);
      bound = torch::stack({-xlo, xhi, -alo, ahi}).max().item<double>();
    }
    gen_f16 = bound < SF_F16_ABS_LIMIT;   // false for NaN
    TORCH_CHECK(gen_f16 || gen == "auto", "gen=\"f16\" needs |Xs| and |As| "
                "below ", SF_F16_ABS_LIMIT, ", got ", bound);
  }
  make_contiguous({&Xs, &As, &nx, &na, &y});
  check_hip(launch_syrk_fused_gen(
                Xs.data_ptr<float>(), As.data_ptr<float>(),
                nx.data_ptr<float>(), na.data_ptr<float>(), (float)amp,
                y.data_ptr<float>(), c, m, d, (int)split_k,
                Ky.data_ptr<double>(), KK.data_ptr<float>(),
                part.data_ptr<float>(), (int)family, gen_f16 ? 1 : 0,
                current_stream()),
            "ppa_fused_acc");
}

void colsum_gemv_acc(torch::Tensor Kc, torch::Tensor y, torch::Tensor Ky) {
  check_arg(Kc, "Kc", BF16, {ANY, ANY});
  const int c = Kc.size(0), m = Kc.size(1);
  check_vec(y, "y", F32, c);
  check_vec(Ky, "Ky", F64, m, true);
  check_same_gpu({{&Kc, "Kc"}, {&y, "y"}, {&Ky, "Ky"}});
  make_contiguous({&Kc, &y});
  check_hip(launch_colsum_gemv(Kc.data_ptr(), y.data_ptr<float>(), c, m,
                               Ky.data_ptr<double>(), current_stream()),
            "colsum_gemv");
}

// The per-expert Laplace Newton loop, run in place on f.
// EV = false: returns (psi[E] f64, sumlogl[E] f64, iters[E] i32, bad[E] i32).
// EV = true: fused Newton + Algorithm 5.1 evidence/gradient (K11) — the
// evidence pass follows in the same launch; returns (logz[E] f64,
// grad[E, d+2] f64 — beta grads then amp then noise, all d(logZ)/d(theta)
// un-negated —, iters[E] i32, bad[E] i32).
// max_newton = 0 skips the Newton loop: f comes back bitwise unchanged and
// iters = 0, and with EV = true the tail evaluates Algorithm 5.1 (logz and
// grad) at the given latent, converged or not — the exit state is recomputed
// at f, nothing is carried over from an iteration.
template <bool EV>
std::vector<torch::Tensor> fused_laplace(torch::Tensor X, torch::Tensor y,
                                         torch::Tensor f, torch::Tensor scale,
                                         double amp, double noise, double tol,
                                         int64_t max_newton) {
  const char* what = EV ? "fused_laplace_evidence" : "fused_laplace_newton";
  check_arg(X, "X", F32, {ANY, ANY, ANY});
  const int E = X.size(0), k = X.size(1), d = X.size(2);
  check_arg(y, "y", F32, {E, k});
  check_arg(f, "f", F32, {E, k}, true);   // updated in place
  check_vec(scale, "scale", F32, d);
  TORCH_CHECK(k <= 128 && d <= k, "X must be [E, k, d] with k<=128, d<=k "
              "for ", what, ", got ", X.sizes());
  check_same_gpu({{&X, "X"}, {&y, "y"}, {&f, "f"}, {&scale, "scale"}});
  make_contiguous({&X, &y, &scale});
  auto psi = torch::empty({E}, like(X, F64)), sll = torch::empty_like(psi);
  auto iters = torch::empty({E}, like(X, I32)), bad = torch::empty_like(iters);
  if (!EV) {
    check_hip(launch_fused_laplace_newton(
                  X.data_ptr<float>(), y.data_ptr<float>(),
                  f.data_ptr<float>(), scale.data_ptr<float>(), (float)amp,
                  (float)noise, E, k, d, tol, (int)max_newton,
                  psi.data_ptr<double>(), sll.data_ptr<double>(),
                  iters.data_ptr<int>(), bad.data_ptr<int>(),
                  current_stream()),
              what);
    return {psi, sll, iters, bad};
  }
  auto logz = torch::empty({E}, like(X, F64));
  auto grad = torch::empty({E, d + 2}, like(X, F64));
  check_hip(launch_fused_laplace_evidence(
                X.data_ptr<float>(), y.data_ptr<float>(),
                f.data_ptr<float>(), scale.data_ptr<float>(), (float)amp,
                (float)noise, E, k, d, tol, (int)max_newton,
                psi.data_ptr<double>(), sll.data_ptr<double>(),
                iters.data_ptr<int>(), bad.data_ptr<int>(),
                logz.data_ptr<double>(), grad.data_ptr<double>(),
                current_stream()),
            what);
  return {logz, grad, iters, bad};
}

bool fused_laplace_newton_supported(int64_t k, int64_t d) {
  if (k > 128 || d > k || k < 1) return false;
  return lap_lds_bytes((int)k, (int)d) <= GEOM_LDS_MAX;
}

bool fused_laplace_evidence_supported(int64_t k, int64_t d) {
  if (k > 128 || d > k || k < 1) return false;
  return lap_lds_bytes((int)k, (int)d, 1) <= GEOM_LDS_MAX;
}

// K14: fused prediction (predict.hip).  mean = c mv and, with want_var,
// var = kxx + rowsum((c M) o c) for c = amp Kb(q(X, A)), without a [t, m]
// array in memory.  M is the symmetric magic matrix; returns (mean[t] f64,
// var[t] f64 or None).
bool ppa_predict_supported(int64_t m, int64_t d) {
  return ppa_predict_supported_md((long)m, (long)d);
}

// test rows per block the launcher picks for m active points (0: refused)
int64_t ppa_predict_tile_rows(int64_t m) {
  return pp_tile_rows((long)m);
}

std::tuple<torch::Tensor, c10::optional<torch::Tensor>> ppa_predict(
    torch::Tensor X, torch::Tensor A, torch::Tensor s2, double amp,
    torch::Tensor mv, torch::Tensor M, double kxx, bool want_var,
    int64_t family) {
  check_family(family);
  check_arg(X, "X", F32, {ANY, ANY});
  const int64_t t = X.size(0), d = X.size(1);
  check_arg(A, "A", F32, {ANY, d});
  const int64_t m = A.size(0);
  check_vec(s2, "s2", F32, d);
  check_arg(mv, "mv", F64, {m});
  check_arg(M, "M", F64, {m, m});
  TORCH_CHECK(ppa_predict_supported(m, d), "A: unsupported (m, d) = (", m,
              ", ", d, ") for ppa_predict; query ppa_predict_supported");
  check_same_gpu({{&X, "X"}, {&A, "A"}, {&s2, "s2"}, {&mv, "mv"}, {&M, "M"}});
  make_contiguous({&X, &A, &s2, &mv, &M});
  auto mean = torch::empty({t}, like(X, F64));
  c10::optional<torch::Tensor> var;
  if (want_var) var = torch::empty({t}, like(X, F64));
  check_hip(launch_ppa_predict(
                X.data_ptr<float>(), A.data_ptr<float>(),
                s2.data_ptr<float>(), (float)amp, mv.data_ptr<double>(),
                M.data_ptr<double>(), kxx, (long)t, (int)m, (int)d,
                mean.data_ptr<double>(),
                want_var ? var->data_ptr<double>() : nullptr, (int)family,
                current_stream()),
            "ppa_predict");
  return {mean, var};
}

// ---------------------------------------------------------------------------
// K13: blocked fp64 Cholesky path (big_chol.hip) — host orchestration
// ---------------------------------------------------------------------------

// In-place blocked Cholesky of the padded [mp, mp] fp64 matrix A (lower
// triangle; strict upper left untouched).  V [nb, 64, 64] receives the
// explicit inverse of each diagonal block; bad (int32 [1], zeroed by the
// caller) is set on a non-PD pivot.  mp must be a multiple of 64.
void dpotrf64(torch::Tensor A, torch::Tensor V, torch::Tensor bad) {
  check_arg(A, "A", F64, {ANY, ANY}, true);
  const long mp = A.size(0), nb = mp / 64;
  TORCH_CHECK(A.size(1) == mp && mp % 64 == 0,
              "A must be square and 64-padded, got ", A.sizes());
  check_vec(V, "V", F64, nb * 64 * 64, true);
  check_vec(bad, "bad", I32, 1);
  check_same_gpu({{&A, "A"}, {&V, "V"}, {&bad, "bad"}});
  auto stream = current_stream();
  double* a = A.data_ptr<double>();
  double* v = V.data_ptr<double>();
  int* bd = bad.data_ptr<int>();
  for (long J = 0; J < nb; ++J) {
    const long jb = J * 64;
    check_hip(launch_dpotrf_diag(a, mp, (int)jb, v + J * 4096, bd, stream),
              "dpotrf_diag");
    const long nr = mp - jb - 64;
    if (nr > 0) {
      double* A21 = a + (size_t)(jb + 64) * mp + jb;
      // panel solve L21 = A21 V_J^T (in place)
      check_hip(launch_dgemm64(0, 1, 0, 0, A21, v + J * 4096, A21,
                               (int)nr, 64, 64, mp, 64, mp, stream),
                "dtrsm_panel");
      // trailing A22 -= L21 L21^T (lower tiles only)
      double* A22 = a + (size_t)(jb + 64) * mp + jb + 64;
      check_hip(launch_dgemm64(0, 1, 1, 1, A21, A21, A22,
                               (int)nr, (int)nr, 64, mp, mp, mp, stream),
                "dsyrk_trailing");
    }
  }
}

// Solve (L L^T) X = B in place on B [mp, r] given the factored A (lower L)
// and the diagonal-block inverses V from dpotrf64.  rhs_identity=true
// declares B to be the identity (the explicit-inverse path): the forward
// pass then skips the provably-zero column range of each block step —
// Y = L^{-1} is lower triangular, so block row I has nonzeros only in
// columns < (I+1)*64 — cutting the forward GEMMs from m^3 to m^3/3.
void dchol_solve64(torch::Tensor A, torch::Tensor V, torch::Tensor B,
                   bool rhs_identity) {
  check_arg(A, "A", F64, {ANY, ANY}, true);
  const long mp = A.size(0), nb = mp / 64;
  TORCH_CHECK(mp % 64 == 0, "A must be 64-padded, got ", A.sizes());
  check_vec(V, "V", F64, nb * 64 * 64, true);
  check_arg(B, "B", F64, {mp, ANY}, true);
  check_same_gpu({{&A, "A"}, {&V, "V"}, {&B, "B"}});
  const long r = B.size(1);
  auto stream = current_stream();
  double* a = A.data_ptr<double>();
  double* v = V.data_ptr<double>();
  double* b = B.data_ptr<double>();
  for (long I = 0; I < nb; ++I) {            // forward: L Y = B
    const long jb = I * 64;
    const long rc = rhs_identity ? std::min<long>(r, jb + 64) : r;
    check_hip(launch_dgemm64(0, 0, 0, 0, v + I * 4096, b + jb * r,
                             b + jb * r, 64, (int)rc, 64, 64, r, r, stream),
              "fwd_diag");
    const long nr = mp - jb - 64;
    if (nr > 0)
      check_hip(launch_dgemm64(0, 0, 1, 0, a + (size_t)(jb + 64) * mp + jb,
                               b + jb * r, b + (jb + 64) * r,
                               (int)nr, (int)rc, 64, mp, r, r, stream),
                "fwd_update");
  }
  for (long I = nb - 1; I >= 0; --I) {       // backward: L^T X = Y
    const long jb = I * 64;
    check_hip(launch_dgemm64(1, 0, 0, 0, v + I * 4096, b + jb * r,
                             b + jb * r, 64, (int)r, 64, 64, r, r, stream),
              "bwd_diag");
    if (jb > 0)
      check_hip(launch_dgemm64(1, 0, 1, 0, a + (size_t)jb * mp, b + jb * r,
                               b, (int)jb, (int)r, 64, mp, r, r, stream),
                "bwd_update");
  }
}

// Generic fp64 MFMA GEMM (layout verification + utility): C = op(A) op(B).
torch::Tensor dgemm64(torch::Tensor A, torch::Tensor B, bool ta, bool tb) {
  check_arg(A, "A", F64, {ANY, ANY});
  check_arg(B, "B", F64, {ANY, ANY});
  const long M = ta ? A.size(1) : A.size(0);
  const long K = ta ? A.size(0) : A.size(1);
  const long Kb = tb ? B.size(1) : B.size(0);
  const long N = tb ? B.size(0) : B.size(1);
  TORCH_CHECK(K == Kb, "inner dims of A and B differ");
  check_same_gpu({{&A, "A"}, {&B, "B"}});
  make_contiguous({&A, &B});
  auto C = torch::empty({M, N}, A.options());
  check_hip(launch_dgemm64(ta ? 1 : 0, tb ? 1 : 0, 0, 0,
                           A.data_ptr<double>(), B.data_ptr<double>(),
                           C.data_ptr<double>(), (int)M, (int)N, (int)K,
                           A.size(1), B.size(1), N, current_stream()),
            "dgemm64");
  return C;
}

// K19: device-side synthetic benchmark data (Philox4x32-10)
std::vector<torch::Tensor> synth_regression(int64_t n, int64_t d,
                                            int64_t seed, double noise_sd) {
  auto dev = torch::TensorOptions().dtype(torch::kFloat32)
                 .device(torch::kCUDA);
  auto X = torch::empty({n, d}, dev);
  auto y = torch::empty({n}, dev);
  check_hip(launch_synth_regression(X.data_ptr<float>(), y.data_ptr<float>(),
                                    n, (int)d, (unsigned long long)seed,
                                    (float)noise_sd, current_stream()),
            "synth_regression");
  return {X, y};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  // kernel geometry the Python plan module mirrors (checked by a test)
  mod.attr("SY_CT") = (int)SY_CT;
  mod.attr("SY_BK") = (int)SY_BK;
  mod.attr("SF_DMAX") = (int)SF_DMAX;
  mod.attr("SY_SPLITK_MAX_TILES") = (int)SY_SPLITK_MAX_TILES;
  mod.attr("SF_F16_ABS_LIMIT") = (double)SF_F16_ABS_LIMIT;
  // covariance family codes of the `family` arguments below
  mod.attr("FAM_RBF") = (int)GEOM_FAM_RBF;
  mod.attr("FAM_M32") = (int)GEOM_FAM_M32;
  mod.attr("FAM_M52") = (int)GEOM_FAM_M52;
  mod.def("synth_regression", &synth_regression,
          "device-side Philox benchmark data (K19)");
  mod.def("dpotrf64", &dpotrf64,
          "blocked fp64 Cholesky (K13), in place, 64-padded");
  mod.def("dchol_solve64", &dchol_solve64,
          "blocked fp64 triangular solves (L L^T) X = B, in place on B",
          pybind11::arg("A"), pybind11::arg("V"), pybind11::arg("B"),
          pybind11::arg("rhs_identity") = false);
  mod.def("dgemm64", &dgemm64, "fp64 MFMA GEMM (test/utility)");
  mod.def("fused_laplace_newton", &fused_laplace<false>,
          "per-expert Laplace Newton loop to convergence (CDNA4)");
  mod.def("fused_laplace_newton_supported", &fused_laplace_newton_supported);
  mod.def("fused_laplace_evidence", &fused_laplace<true>,
          "fused Newton + Algorithm 5.1 evidence/gradient (K11, CDNA4)");
  mod.def("fused_laplace_evidence_supported",
          &fused_laplace_evidence_supported);
  mod.def("fused_expert_nll", &fused_expert_nll,
          "fused per-expert BCM nll+gradient primitives (CDNA4)",
          pybind11::arg("X"), pybind11::arg("y"), pybind11::arg("scale"), pybind11::arg("amp"), pybind11::arg("noise"),
          pybind11::arg("family") = (int)GEOM_FAM_RBF);
  mod.def("fused_expert_nll_profile", &fused_expert_nll_impl,
          "same, with per-phase wall_clock64 boundaries appended",
          pybind11::arg("X"), pybind11::arg("y"), pybind11::arg("scale"), pybind11::arg("amp"), pybind11::arg("noise"),
          pybind11::arg("profile"), pybind11::arg("family") = (int)GEOM_FAM_RBF);
  mod.def("fused_expert_nll_supported", &fused_expert_nll_supported);
  mod.def("fused_expert_nll_occupancy", &fused_expert_nll_occupancy,
          "resident workgroups per CU of the expert kernel at (k, d)",
          pybind11::arg("k"), pybind11::arg("d"), pybind11::arg("family") = (int)GEOM_FAM_RBF);
  mod.def("cross_mfma_ppa", &cross_mfma_ppa,
          "MFMA sqdist cross tile + fused K^T y (K1 plan, CDNA4)",
          pybind11::arg("Xs"), pybind11::arg("As"), pybind11::arg("nx"), pybind11::arg("na"), pybind11::arg("amp"), pybind11::arg("y"),
          pybind11::arg("Ky"), pybind11::arg("family") = (int)GEOM_FAM_RBF);
  mod.def("ppa_fused_acc", &ppa_fused_acc,
          "KK += K^T K, Ky += K^T y with K_nm generated in the SYRK (CDNA4)",
          pybind11::arg("Xs"), pybind11::arg("As"), pybind11::arg("nx"), pybind11::arg("na"), pybind11::arg("amp"), pybind11::arg("y"),
          pybind11::arg("Ky"), pybind11::arg("KK"), pybind11::arg("split_k"),
          pybind11::arg("family") = (int)GEOM_FAM_RBF,
          pybind11::arg("gen") = "auto",
          pybind11::arg("absmax") = pybind11::none(),
          pybind11::arg("partials") = pybind11::none());
  mod.def("ppa_fused_partials_numel",
          [](int64_t c, int64_t m, int64_t split_k) {
            return (int64_t)sf_partial_floats(c, m, split_k);
          },
          "fp32 elements of ppa_fused_acc's partials buffer",
          pybind11::arg("c"), pybind11::arg("m"), pybind11::arg("split_k"));
  mod.def("ppa_fused_supported", &ppa_fused_supported);
  mod.def("cross_kernel_tile_ppa", &cross_kernel_tile_ppa,
          "transposed hi/lo tiles + fused K^T y accumulation (CDNA4)",
          pybind11::arg("X"), pybind11::arg("A"), pybind11::arg("s2v"), pybind11::arg("amp"), pybind11::arg("y"), pybind11::arg("Ky"),
          pybind11::arg("family") = (int)GEOM_FAM_RBF);
  mod.def("cross_kernel_tile", &cross_kernel_tile,
          "rectangular kernel block of a covariance family (CDNA4)",
          pybind11::arg("X"), pybind11::arg("A"), pybind11::arg("s2v"),
          pybind11::arg("amp"), pybind11::arg("bf16_out"),
          pybind11::arg("hilo"), pybind11::arg("want_t") = false,
          pybind11::arg("family") = (int)GEOM_FAM_RBF);
  mod.def("ppa_predict", &ppa_predict,
          "fused cross kernel + predictive mean and variance (K14, CDNA4)",
          pybind11::arg("X"), pybind11::arg("A"), pybind11::arg("s2"),
          pybind11::arg("amp"), pybind11::arg("mv"), pybind11::arg("M"),
          pybind11::arg("kxx"), pybind11::arg("want_var"),
          pybind11::arg("family") = (int)GEOM_FAM_RBF);
  mod.def("ppa_predict_supported", &ppa_predict_supported);
  mod.def("ppa_predict_tile_rows", &ppa_predict_tile_rows,
          "test rows per block of ppa_predict at m active points (0: none)");
  mod.def("syrk_bf16_sync_acc", &syrk_bf16_sync_acc,
          "k-synchronized persistent SYRK for large m (CDNA4)");
  mod.def("syrk_bf16_acc", &syrk_bf16_acc,
          "KK += K K^T of the transposed block KcT [m, c]; bf16 MFMA, "
          "fp32 accumulate (CDNA4)");
  mod.def("colsum_gemv_acc", &colsum_gemv_acc,
          "Ky += Kc^T y, fp64 accumulate (CDNA4)");
}
