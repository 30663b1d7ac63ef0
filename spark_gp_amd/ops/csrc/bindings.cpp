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

// The same five outputs for experts of 128 < k <= 1024 rows
// (expert_nll_panel.hip).  Persistent workgroups keep the matrix of the
// expert they are on in a scratch of grid x kp x kp floats, allocated here:
// grid = min(E, resident workgroups, what NLP_SCRATCH_MAX_BYTES holds,
// max_blocks if > 0), so it never grows with E.  The kernel reads X in
// place: a non-contiguous X is refused, not copied.  sb: the super-block, 64
// or 128 (0: nlp_sb_default(k)); an expert's outputs depend on sb, never on
// the grid.
bool fused_expert_nll_panel_supported(int64_t k, int64_t d) {
  return nlp_supported_kd((long)k, (long)d) &&
         nlp_lds_bytes(64, (int)k, (int)d) <= GEOM_LDS_MAX &&
         nlp_lds_bytes(128, (int)k, (int)d) <= GEOM_LDS_MAX;
}

int64_t fused_expert_nll_panel_scratch_bytes(int64_t grid, int64_t k,
                                             int64_t sb) {
  if (sb == 0) sb = nlp_sb_default((long)k);
  TORCH_CHECK(nlp_sb_ok(sb), "sb must be 64 or 128 (0: default), got ", sb);
  TORCH_CHECK(k >= 1 && k <= NLP_K_MAX && grid >= 0, "k must be in [1, ",
              NLP_K_MAX, "] and grid >= 0, got k = ", k, ", grid = ", grid);
  return (int64_t)(nlp_scratch_floats((long)grid, (int)k, (int)sb) *
                   sizeof(float));
}

std::vector<torch::Tensor> fused_expert_nll_panel(
    torch::Tensor X, torch::Tensor y, torch::Tensor scale, double amp,
    double noise, int64_t family, int64_t max_blocks, int64_t sb) {
  check_family(family);
  check_arg(X, "X", F32, {ANY, ANY, ANY}, true);
  const int E = X.size(0), k = X.size(1), d = X.size(2);
  check_arg(y, "y", F32, {E, k});
  check_vec(scale, "scale", F32, d);
  TORCH_CHECK(fused_expert_nll_panel_supported(k, d), "X must be [E, k, d] "
              "with 128 < k <= 1024, 1 <= d <= 128 for "
              "fused_expert_nll_panel, got ", X.sizes());
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0 (0: no cap), got ",
              max_blocks);
  if (sb == 0) sb = nlp_sb_default(k);
  TORCH_CHECK(nlp_sb_ok(sb), "sb must be 64 or 128 (0: default), got ", sb);
  check_same_gpu({{&X, "X"}, {&y, "y"}, {&scale, "scale"}});
  make_contiguous({&y, &scale});
  auto nll = torch::empty({E}, like(X, F64));
  auto sumW0 = torch::empty_like(nll), trG = torch::empty_like(nll);
  auto contr = torch::empty({E, d}, like(X, F64));
  auto bad = torch::empty({E}, like(X, I32));
  if (E == 0) return {nll, sumW0, trG, contr, bad};
  int cus = 0, wgs = 0;
  check_hip(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                  X.get_device()),
            "fused_expert_nll_panel: compute unit count");
  check_hip(fused_expert_nll_panel_resident_wgs(k, d, (int)family, (int)sb,
                                                &wgs),
            "fused_expert_nll_panel: occupancy");
  TORCH_CHECK(cus >= 1 && wgs >= 1, "fused_expert_nll_panel: the device "
              "keeps no workgroup resident at (k, d) = (", k, ", ", d, ")");
  const long grid = nlp_grid(E, (long)cus * wgs, (long)max_blocks, k,
                             (int)sb);
  const size_t floats = nlp_scratch_floats(grid, k, (int)sb);
  TORCH_CHECK(grid >= 1 && floats * sizeof(float) <= NLP_SCRATCH_MAX_BYTES,
              "fused_expert_nll_panel: scratch of ", floats * sizeof(float),
              " bytes for ", grid, " workgroups is outside the limit of ",
              NLP_SCRATCH_MAX_BYTES);
  // every element a phase reads has been written by an earlier phase of the
  // same expert: no clearing
  auto scratch = torch::empty({(int64_t)floats}, like(X, F32));
  check_hip(launch_fused_expert_nll_panel(
                X.data_ptr<float>(), y.data_ptr<float>(),
                scale.data_ptr<float>(), (float)amp, (float)noise, E, k, d,
                scratch.data_ptr<float>(), (int)grid, (int)sb,
                nll.data_ptr<double>(), sumW0.data_ptr<double>(),
                trG.data_ptr<double>(), contr.data_ptr<double>(),
                bad.data_ptr<int>(), (int)family, current_stream()),
            "fused_expert_nll_panel");
  return {nll, sumW0, trG, contr, bad};
}

// The same five outputs in full fp64 for k <= 128, d <= 128
// (expert_nll_f64.hip): X fp32 or fp64, widened at the load and read in
// place (a non-contiguous X is refused, not copied); y and the scale vector
// fp64, since an fp32 scale would cap the result at 1e-7.
bool fused_expert_nll_f64_supported(int64_t k, int64_t d) {
  return nllf64_supported((long)k, (long)d);
}

std::vector<torch::Tensor> fused_expert_nll_f64(
    torch::Tensor X, torch::Tensor y, torch::Tensor scale, double amp,
    double noise, int64_t family) {
  check_family(family);
  const bool x64 = X.scalar_type() == F64;
  check_arg(X, "X", x64 ? F64 : F32, {ANY, ANY, ANY}, true);
  const int E = X.size(0), k = X.size(1), d = X.size(2);
  check_arg(y, "y", F64, {E, k});
  check_vec(scale, "scale", F64, d);
  TORCH_CHECK(fused_expert_nll_f64_supported(k, d), "X must be [E, k, d] "
              "with 1 <= k <= 128, 1 <= d <= 128 for fused_expert_nll_f64, "
              "got ", X.sizes());
  check_same_gpu({{&X, "X"}, {&y, "y"}, {&scale, "scale"}});
  make_contiguous({&y, &scale});
  auto nll = torch::empty({E}, like(X, F64));
  auto sumW0 = torch::empty_like(nll), trG = torch::empty_like(nll);
  auto contr = torch::empty({E, d}, like(X, F64));
  auto bad = torch::empty({E}, like(X, I32));
  if (E == 0) return {nll, sumW0, trG, contr, bad};
  check_hip(launch_fused_expert_nll_f64(
                X.data_ptr(), x64 ? 1 : 0, y.data_ptr<double>(),
                scale.data_ptr<double>(), amp, noise, E, k, d,
                nll.data_ptr<double>(), sumW0.data_ptr<double>(),
                trG.data_ptr<double>(), contr.data_ptr<double>(),
                bad.data_ptr<int>(), (int)family, current_stream()),
            "fused_expert_nll_f64");
  return {nll, sumW0, trG, contr, bad};
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

// Fused fp64 PPA accumulation (ppa_fp64.hip): KK [m, m] += K^T K and
// Ky [m] += K^T y with fp32 kernel values and fp64 products and sums, both
// triangles of KK written, the same bits on every run.
//
// With A (and s2): X is the fp32 rows [c, d], d <= PF_DMAX, and the blocks
// generate K = amp Kb(sum_j s2_j (x_j - a_j)^2) themselves.  Without: X is
// the fp32 chunk K [c, m] (cross_kernel_tile's output) and s2, amp and
// family are not used.
//
// partials: scratch of ppa_fp64_partials_numel(m, split_k) doubles or more,
// contents irrelevant; allocated here when absent and needed (split_k > 1).
bool ppa_fp64_supported(int64_t m, int64_t d) {
  return ppa_fp64_supported_md(m, d);
}

void ppa_fp64_acc(torch::Tensor X, torch::Tensor y, torch::Tensor Ky,
                  torch::Tensor KK, int64_t split_k,
                  c10::optional<torch::Tensor> A,
                  c10::optional<torch::Tensor> s2, double amp, int64_t family,
                  c10::optional<torch::Tensor> partials) {
  check_family(family);
  check_arg(X, "X", F32, {ANY, ANY});
  const bool gen = A.has_value();
  TORCH_CHECK(gen == s2.has_value(), "A and s2 come together");
  if (gen) {
    check_arg(*A, "A", F32, {ANY, X.size(1)});
    check_vec(*s2, "s2", F32, X.size(1));
  }
  const int64_t c = X.size(0), m = gen ? A->size(0) : X.size(1);
  const int64_t d = gen ? X.size(1) : 1;
  TORCH_CHECK(ppa_fp64_supported(m, d) && (!gen || d <= PF_DMAX),
              "X: unsupported (m, d) = (", m, ", ", d, ") for ppa_fp64_acc; "
              "query ppa_fp64_supported, and generate for d <= ", PF_DMAX);
  TORCH_CHECK(c <= (1 << 30), "X: at most 2^30 rows per call, got ", c);
  check_vec(y, "y", F32, c);
  check_vec(Ky, "Ky", F64, m, true);
  check_arg(KK, "KK", F64, {m, m}, true);
  TORCH_CHECK(split_k >= 1 && split_k * pf_tiles(m) <= INT_MAX,
              "split_k out of range [1, ", INT_MAX / pf_tiles(m), "]: ",
              split_k);
  const int64_t part_doubles = (int64_t)pf_partial_doubles(m, split_k);
  if (partials.has_value()) {
    check_dtype(*partials, "partials", F64, true);
    TORCH_CHECK(partials->numel() >= part_doubles, "partials must have at "
                "least ", part_doubles, " elements for this (m, split_k), "
                "got ", partials->numel());
  }
  check_same_gpu({{&X, "X"}, {&y, "y"}, {&Ky, "Ky"}, {&KK, "KK"},
                  {gen ? &*A : nullptr, "A"}, {gen ? &*s2 : nullptr, "s2"},
                  {partials.has_value() ? &*partials : nullptr, "partials"}});
  if (c == 0) return;
  torch::Tensor part = partials.has_value()
                           ? *partials
                           : torch::empty({part_doubles}, like(KK, F64));
  torch::Tensor Ac, s2c;
  make_contiguous({&X, &y});
  if (gen) {
    Ac = A->contiguous();
    s2c = s2->contiguous();
  }
  check_hip(launch_ppa_fp64(
                X.data_ptr<float>(), gen ? Ac.data_ptr<float>() : nullptr,
                gen ? s2c.data_ptr<float>() : nullptr, (float)amp,
                y.data_ptr<float>(), (int)c, (int)m, (int)d, (int)split_k,
                Ky.data_ptr<double>(), KK.data_ptr<double>(),
                part_doubles ? part.data_ptr<double>() : nullptr,
                (int)family, current_stream()),
            "ppa_fp64_acc");
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

// the response link code of a fused Laplace entry point (kernel_geom.h)
void check_link(int64_t link) {
  TORCH_CHECK(lap_link_ok(link), "link must be 0 (logistic) or 1 (probit), "
              "got ", link);
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
// family: the covariance family of the base kernel (default RBF).
// link: the response link (default logistic); probit is built for the RBF
// family only.
template <bool EV>
std::vector<torch::Tensor> fused_laplace(torch::Tensor X, torch::Tensor y,
                                         torch::Tensor f, torch::Tensor scale,
                                         double amp, double noise, double tol,
                                         int64_t max_newton, int64_t family,
                                         int64_t link) {
  const char* what = EV ? "fused_laplace_evidence" : "fused_laplace_newton";
  check_family(family);
  check_link(link);
  TORCH_CHECK(link == LAP_LINK_LOGISTIC || family == GEOM_FAM_RBF,
              "the probit link takes the RBF family only, got family ",
              family, " for ", what);
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
                  iters.data_ptr<int>(), bad.data_ptr<int>(), (int)family,
                  (int)link, current_stream()),
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
                (int)family, (int)link, current_stream()),
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

// The two entries above on laplace_wide.hip, which streams X instead of
// holding it in LDS: RBF family, 1 <= k <= 128, 1 <= d <= 1024 (d > k
// included).  Same tuples, same max_newton = 0 contract.  X must be
// contiguous: the experts are large, and a silent copy of them per call
// would cost more than the launch.
bool fused_laplace_wide_supported(int64_t k, int64_t d) {
  return lapw_supported((long)k, (long)d, 1);
}

// workgroups of the wide evidence kernel that one CU keeps resident
int64_t fused_laplace_wide_occupancy(int64_t k, int64_t d) {
  int wgs = 0;
  check_hip(fused_laplace_wide_resident_wgs((int)k, (int)d, &wgs),
            "fused_laplace_wide_occupancy");
  return wgs;
}

template <bool EV>
std::vector<torch::Tensor> fused_laplace_wide(
    torch::Tensor X, torch::Tensor y, torch::Tensor f, torch::Tensor scale,
    double amp, double noise, double tol, int64_t max_newton, int64_t link) {
  const char* what =
      EV ? "fused_laplace_evidence_wide" : "fused_laplace_newton_wide";
  check_link(link);
  check_arg(X, "X", F32, {ANY, ANY, ANY}, true);
  const int E = X.size(0), k = X.size(1), d = X.size(2);
  check_arg(y, "y", F32, {E, k});
  check_arg(f, "f", F32, {E, k}, true);   // updated in place
  check_vec(scale, "scale", F32, d);
  TORCH_CHECK(fused_laplace_wide_supported(k, d), "X must be [E, k, d] with "
              "1<=k<=128, 1<=d<=", LAPW_D_MAX, " for ", what, ", got ",
              X.sizes());
  check_same_gpu({{&X, "X"}, {&y, "y"}, {&f, "f"}, {&scale, "scale"}});
  make_contiguous({&y, &scale});
  auto psi = torch::empty({E}, like(X, F64)), sll = torch::empty_like(psi);
  auto iters = torch::empty({E}, like(X, I32)), bad = torch::empty_like(iters);
  if (!EV) {
    check_hip(launch_fused_laplace_newton_wide(
                  X.data_ptr<float>(), y.data_ptr<float>(),
                  f.data_ptr<float>(), scale.data_ptr<float>(), (float)amp,
                  (float)noise, E, k, d, tol, (int)max_newton,
                  psi.data_ptr<double>(), sll.data_ptr<double>(),
                  iters.data_ptr<int>(), bad.data_ptr<int>(), (int)link,
                  current_stream()),
              what);
    return {psi, sll, iters, bad};
  }
  auto logz = torch::empty({E}, like(X, F64));
  auto grad = torch::empty({E, d + 2}, like(X, F64));
  check_hip(launch_fused_laplace_evidence_wide(
                X.data_ptr<float>(), y.data_ptr<float>(),
                f.data_ptr<float>(), scale.data_ptr<float>(), (float)amp,
                (float)noise, E, k, d, tol, (int)max_newton,
                psi.data_ptr<double>(), sll.data_ptr<double>(),
                iters.data_ptr<int>(), bad.data_ptr<int>(),
                logz.data_ptr<double>(), grad.data_ptr<double>(), (int)link,
                current_stream()),
            what);
  return {logz, grad, iters, bad};
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

// K14, wide form (predict_wide.hip): the same outputs for 1 <= m <=
// PPW_M_MAX.  Persistent blocks over 128-row tiles keep the cross rows in a
// scratch buffer of grid x 128 x mp floats, allocated here: bounded by the
// grid (one block per compute unit; max_blocks > 0 caps it), never by t.
bool ppa_predict_wide_supported(int64_t m, int64_t d) {
  return ppa_predict_wide_supported_md((long)m, (long)d);
}

std::tuple<torch::Tensor, c10::optional<torch::Tensor>> ppa_predict_wide(
    torch::Tensor X, torch::Tensor A, torch::Tensor s2, double amp,
    torch::Tensor mv, torch::Tensor M, double kxx, bool want_var,
    int64_t family, int64_t max_blocks) {
  check_family(family);
  check_arg(X, "X", F32, {ANY, ANY});
  const int64_t t = X.size(0), d = X.size(1);
  check_arg(A, "A", F32, {ANY, d});
  const int64_t m = A.size(0);
  check_vec(s2, "s2", F32, d);
  check_arg(mv, "mv", F64, {m});
  check_arg(M, "M", F64, {m, m});
  TORCH_CHECK(ppa_predict_wide_supported(m, d), "A: unsupported (m, d) = (",
              m, ", ", d,
              ") for ppa_predict_wide; query ppa_predict_wide_supported");
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0 (0: no cap), got ",
              max_blocks);
  check_same_gpu({{&X, "X"}, {&A, "A"}, {&s2, "s2"}, {&mv, "mv"}, {&M, "M"}});
  make_contiguous({&X, &A, &s2, &mv, &M});
  auto mean = torch::empty({t}, like(X, F64));
  c10::optional<torch::Tensor> var;
  if (want_var) var = torch::empty({t}, like(X, F64));
  int cus = 0;
  check_hip(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                  X.get_device()),
            "ppa_predict_wide: compute unit count");
  const long grid = ppw_grid((long)t, cus, (long)max_blocks);
  torch::Tensor scratch;
  if (want_var)
    scratch = torch::empty({(int64_t)ppw_scratch_floats(grid, (int)m)},
                           like(X, F32));
  check_hip(launch_ppa_predict_wide(
                X.data_ptr<float>(), A.data_ptr<float>(),
                s2.data_ptr<float>(), (float)amp, mv.data_ptr<double>(),
                M.data_ptr<double>(), kxx, (long)t, (int)m, (int)d,
                want_var ? scratch.data_ptr<float>() : nullptr, (int)grid,
                mean.data_ptr<double>(),
                want_var ? var->data_ptr<double>() : nullptr, (int)family,
                current_stream()),
            "ppa_predict_wide");
  return {mean, var};
}

// K15: incremental greedy forward selection (greedy.hip).  The caller owns
// the state of a selection of m points among n rows: U fp32 and V fp64
// [m, n_pad], row vectors of n_pad = greedy_npad(n) elements (y zero past
// n; p, q, mu zero before the first round), partials
// [greedy_blocks(n), m + 2].  A round with mc points already in runs pass 1,
// then (after the host's step on sums) pass 2; both write the state in place.
bool greedy_supported(int64_t n, int64_t m, int64_t d) {
  return greedy_supported_nmd((long)n, (long)m, (long)d);
}

static void check_greedy_state(const torch::Tensor& S, const char* name,
                               torch::ScalarType dtype, int64_t n,
                               int64_t mc) {
  check_arg(S, name, dtype, {ANY, (int64_t)gr_npad((long)n)}, true);
  TORCH_CHECK(mc >= 0 && mc < S.size(0), "mc must be in [0, ", S.size(0),
              ") for ", name, " of ", S.size(0), " columns, got ", mc);
}

// sums[:mc] = V[:mc] c, sums[mc] = c.c, sums[mc + 1] = c.y for the fp32
// column c = amp Kb(q(X, xstar)), which is stored; U[mc] and p are updated.
void greedy_pass1(torch::Tensor X, torch::Tensor xstar, torch::Tensor s2,
                  double amp, torch::Tensor y, torch::Tensor a, double a_nn,
                  int64_t mc, torch::Tensor U, torch::Tensor V,
                  torch::Tensor c, torch::Tensor p, torch::Tensor partials,
                  torch::Tensor sums, int64_t family) {
  check_family(family);
  check_arg(X, "X", F32, {ANY, ANY});
  const int64_t n = X.size(0), d = X.size(1);
  check_vec(xstar, "xstar", F32, d);
  check_vec(s2, "s2", F32, d);
  TORCH_CHECK(U.dim() == 2 && greedy_supported(n, U.size(0), d),
              "unsupported (n, m, d) = (", n, ", ", U.dim() == 2 ? U.size(0)
              : -1, ", ", d, ") for greedy_pass1; query greedy_supported");
  const int64_t m = U.size(0), np = gr_npad((long)n);
  check_greedy_state(U, "U", F32, n, mc);
  check_greedy_state(V, "V", F64, n, mc);
  TORCH_CHECK(V.size(0) == m, "V must have U's ", m, " columns, got ",
              V.size(0));
  check_arg(y, "y", F64, {np});
  check_arg(a, "a", F64, {mc});
  check_arg(c, "c", F32, {np}, true);
  check_arg(p, "p", F64, {np}, true);
  check_arg(partials, "partials", F64,
            {(int64_t)gr_blocks((long)n), (int64_t)gr_pstride((long)m)}, true);
  check_arg(sums, "sums", F64, {mc + 2}, true);
  check_same_gpu({{&X, "X"}, {&xstar, "xstar"}, {&s2, "s2"}, {&y, "y"},
                  {&a, "a"}, {&U, "U"}, {&V, "V"}, {&c, "c"}, {&p, "p"},
                  {&partials, "partials"}, {&sums, "sums"}});
  make_contiguous({&X, &xstar, &s2, &y, &a});
  check_hip(launch_greedy_pass1(
                X.data_ptr<float>(), xstar.data_ptr<float>(),
                s2.data_ptr<float>(), (float)amp, y.data_ptr<double>(),
                (const double*)a.data_ptr(), a_nn, (long)n, (int)d, (int)mc,
                (int)m, U.data_ptr<float>(), V.data_ptr<double>(),
                c.data_ptr<float>(), p.data_ptr<double>(),
                partials.data_ptr<double>(), sums.data_ptr<double>(),
                (int)family, current_stream()),
            "greedy_pass1");
}

// V[mc], q and mu are updated; delta [n_pad] gets the scores (-inf past n)
// and best = (max score, its lowest row).
void greedy_pass2(torch::Tensor c, torch::Tensor y, torch::Tensor l,
                  double l_nn, double beta_new, double kxx, double sigma2,
                  int64_t n, int64_t mc, torch::Tensor V, torch::Tensor p,
                  torch::Tensor q, torch::Tensor mu, torch::Tensor delta,
                  torch::Tensor bval, torch::Tensor bidx,
                  torch::Tensor best) {
  TORCH_CHECK(V.dim() == 2 && greedy_supported(n, V.size(0), 1),
              "unsupported (n, m) = (", n, ", ", V.dim() == 2 ? V.size(0)
              : -1, ") for greedy_pass2; query greedy_supported");
  const int64_t m = V.size(0), np = gr_npad((long)n);
  const int64_t nb = gr_blocks((long)n);
  check_greedy_state(V, "V", F64, n, mc);
  check_arg(c, "c", F32, {np});
  check_arg(y, "y", F64, {np});
  check_arg(l, "l", F64, {mc});
  check_arg(p, "p", F64, {np});
  check_arg(q, "q", F64, {np}, true);
  check_arg(mu, "mu", F64, {np}, true);
  check_arg(delta, "delta", F64, {np}, true);
  check_arg(bval, "bval", F64, {nb}, true);
  check_arg(bidx, "bidx", torch::kInt64, {nb}, true);
  check_arg(best, "best", F64, {2}, true);
  check_same_gpu({{&c, "c"}, {&y, "y"}, {&l, "l"}, {&V, "V"}, {&p, "p"},
                  {&q, "q"}, {&mu, "mu"}, {&delta, "delta"},
                  {&bval, "bval"}, {&bidx, "bidx"}, {&best, "best"}});
  make_contiguous({&c, &y, &l, &p});
  check_hip(launch_greedy_pass2(
                c.data_ptr<float>(), y.data_ptr<double>(),
                (const double*)l.data_ptr(), l_nn, beta_new, kxx, sigma2,
                (long)n, (int)mc, (int)m, V.data_ptr<double>(),
                p.data_ptr<double>(), q.data_ptr<double>(),
                mu.data_ptr<double>(), delta.data_ptr<double>(),
                bval.data_ptr<double>(), (long long*)bidx.data_ptr<int64_t>(),
                best.data_ptr<double>(), current_stream()),
            "greedy_pass2");
}

// K16: one k-means Lloyd step (kmeans.hip).  The caller owns the work
// buffers, so a loop of steps allocates them once: assign [kmeans_npad(n)]
// int32, c2 [kmeans_mpad(m)] fp32 and partials [kmeans_partial_doubles(n, m,
// d)] fp64 are scratch, sums [m, d] and counts [m] fp64 the result.
bool kmeans_supported(int64_t n, int64_t m, int64_t d) {
  return kmeans_supported_nmd((long)n, (long)m, (long)d);
}

// X's shape, checked against the gate; the rows are read in place
static void check_kmeans_rows(const torch::Tensor& X, int64_t m,
                              const char* what) {
  check_arg(X, "X", F32, {ANY, ANY}, true);
  TORCH_CHECK(kmeans_supported(X.size(0), m, X.size(1)),
              "unsupported (n, m, d) = (", X.size(0), ", ", m, ", ",
              X.size(1), ") for ", what, "; query kmeans_supported");
}

// assign[i] = argmin_j ||c_j||^2 - 2 x_i.c_j, the lowest j among equal
// scores; -1 past n
void kmeans_assign(torch::Tensor X, torch::Tensor centers, torch::Tensor c2,
                   torch::Tensor assign) {
  TORCH_CHECK(centers.dim() == 2, "centers must be [m, d], got ",
              centers.sizes());
  const int64_t m = centers.size(0);
  check_kmeans_rows(X, m, "kmeans_assign");
  const int64_t n = X.size(0), d = X.size(1);
  check_arg(centers, "centers", F32, {m, d});
  check_arg(c2, "c2", F32, {(int64_t)km_mpad((int)m)}, true);
  check_arg(assign, "assign", I32, {(int64_t)km_npad((long)n)}, true);
  check_same_gpu({{&X, "X"}, {&centers, "centers"}, {&c2, "c2"},
                  {&assign, "assign"}});
  make_contiguous({&centers});
  check_hip(launch_kmeans_assign(X.data_ptr<float>(),
                                 centers.data_ptr<float>(), (long)n, (int)m,
                                 (int)d, c2.data_ptr<float>(),
                                 assign.data_ptr<int>(), current_stream()),
            "kmeans_assign");
}

// sums[j] = sum of the rows with assign == j, counts[j] their number; a row
// whose assign is outside [0, m) counts nowhere
void kmeans_accumulate(torch::Tensor X, torch::Tensor assign,
                       torch::Tensor partials, torch::Tensor sums,
                       torch::Tensor counts) {
  TORCH_CHECK(sums.dim() == 2, "sums must be [m, d], got ", sums.sizes());
  const int64_t m = sums.size(0);
  check_kmeans_rows(X, m, "kmeans_accumulate");
  const int64_t n = X.size(0), d = X.size(1);
  check_arg(assign, "assign", I32, {(int64_t)km_npad((long)n)}, true);
  check_arg(partials, "partials", F64,
            {(int64_t)km_partial_doubles((long)n, (long)m, (long)d)}, true);
  check_arg(sums, "sums", F64, {m, d}, true);
  check_arg(counts, "counts", F64, {m}, true);
  check_same_gpu({{&X, "X"}, {&assign, "assign"}, {&partials, "partials"},
                  {&sums, "sums"}, {&counts, "counts"}});
  check_hip(launch_kmeans_accumulate(
                X.data_ptr<float>(), assign.data_ptr<int>(), (long)n, (int)m,
                (int)d, partials.data_ptr<double>(), sums.data_ptr<double>(),
                counts.data_ptr<double>(), current_stream()),
            "kmeans_accumulate");
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
  // response link codes of the `link` arguments of the fused Laplace entries
  mod.attr("LINK_LOGISTIC") = (int)LAP_LINK_LOGISTIC;
  mod.attr("LINK_PROBIT") = (int)LAP_LINK_PROBIT;
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
          "per-expert Laplace Newton loop to convergence (CDNA4)",
          pybind11::arg("X"), pybind11::arg("y"), pybind11::arg("f"), pybind11::arg("scale"), pybind11::arg("amp"),
          pybind11::arg("noise"), pybind11::arg("tol"), pybind11::arg("max_newton"),
          pybind11::arg("family") = (int)GEOM_FAM_RBF,
          pybind11::arg("link") = (int)LAP_LINK_LOGISTIC);
  mod.def("fused_laplace_newton_supported", &fused_laplace_newton_supported);
  mod.def("fused_laplace_evidence", &fused_laplace<true>,
          "fused Newton + Algorithm 5.1 evidence/gradient (K11, CDNA4)",
          pybind11::arg("X"), pybind11::arg("y"), pybind11::arg("f"), pybind11::arg("scale"), pybind11::arg("amp"),
          pybind11::arg("noise"), pybind11::arg("tol"), pybind11::arg("max_newton"),
          pybind11::arg("family") = (int)GEOM_FAM_RBF,
          pybind11::arg("link") = (int)LAP_LINK_LOGISTIC);
  mod.def("fused_laplace_evidence_supported",
          &fused_laplace_evidence_supported);
  mod.def("fused_laplace_newton_wide", &fused_laplace_wide<false>,
          "fused_laplace_newton with X streamed: d up to 1024, d > k allowed",
          pybind11::arg("X"), pybind11::arg("y"), pybind11::arg("f"), pybind11::arg("scale"), pybind11::arg("amp"),
          pybind11::arg("noise"), pybind11::arg("tol"), pybind11::arg("max_newton"),
          pybind11::arg("link") = (int)LAP_LINK_LOGISTIC);
  mod.def("fused_laplace_evidence_wide", &fused_laplace_wide<true>,
          "fused_laplace_evidence with X streamed: d up to 1024, d > k allowed",
          pybind11::arg("X"), pybind11::arg("y"), pybind11::arg("f"), pybind11::arg("scale"), pybind11::arg("amp"),
          pybind11::arg("noise"), pybind11::arg("tol"), pybind11::arg("max_newton"),
          pybind11::arg("link") = (int)LAP_LINK_LOGISTIC);
  mod.def("fused_laplace_wide_supported", &fused_laplace_wide_supported);
  mod.def("fused_laplace_wide_occupancy", &fused_laplace_wide_occupancy);
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
  mod.def("fused_expert_nll_panel", &fused_expert_nll_panel,
          "fused per-expert nll+gradient primitives for 128 < k <= 1024: "
          "the matrix in a global scratch, tiled through LDS (CDNA4)",
          pybind11::arg("X"), pybind11::arg("y"), pybind11::arg("scale"), pybind11::arg("amp"), pybind11::arg("noise"),
          pybind11::arg("family") = (int)GEOM_FAM_RBF,
          pybind11::arg("max_blocks") = 0, pybind11::arg("sb") = 0);
  mod.def("fused_expert_nll_panel_supported",
          &fused_expert_nll_panel_supported);
  mod.def("fused_expert_nll_panel_scratch_bytes",
          &fused_expert_nll_panel_scratch_bytes,
          "bytes of the scratch of a launch of `grid` workgroups",
          pybind11::arg("grid"), pybind11::arg("k"), pybind11::arg("sb") = 0);
  mod.def("fused_expert_nll_f64", &fused_expert_nll_f64,
          "fused per-expert nll+gradient primitives in full fp64 on the f64 "
          "matrix cores, k <= 128 (CDNA4)",
          pybind11::arg("X"), pybind11::arg("y"), pybind11::arg("scale"), pybind11::arg("amp"), pybind11::arg("noise"),
          pybind11::arg("family") = (int)GEOM_FAM_RBF);
  mod.def("fused_expert_nll_f64_supported", &fused_expert_nll_f64_supported);
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
  mod.attr("PF_TILE") = (int)PF_TILE;
  mod.attr("PF_BK") = (int)PF_BK;
  mod.attr("PF_DMAX") = (int)PF_DMAX;
  mod.attr("PF_M_MAX") = (int)PF_M_MAX;
  mod.def("ppa_fp64_acc", &ppa_fp64_acc,
          "KK += K^T K, Ky += K^T y in fp64 on the f64 matrix cores; K "
          "generated from (X, A, s2) or read from the fp32 chunk X (CDNA4)",
          pybind11::arg("X"), pybind11::arg("y"), pybind11::arg("Ky"),
          pybind11::arg("KK"), pybind11::arg("split_k"),
          pybind11::arg("A") = pybind11::none(),
          pybind11::arg("s2") = pybind11::none(),
          pybind11::arg("amp") = 1.0,
          pybind11::arg("family") = (int)GEOM_FAM_RBF,
          pybind11::arg("partials") = pybind11::none());
  mod.def("ppa_fp64_partials_numel",
          [](int64_t m, int64_t split_k) {
            return (int64_t)pf_partial_doubles(m, split_k);
          },
          "fp64 elements of ppa_fp64_acc's partials buffer",
          pybind11::arg("m"), pybind11::arg("split_k"));
  mod.def("ppa_fp64_supported", &ppa_fp64_supported);
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
  mod.def("ppa_predict_wide", &ppa_predict_wide,
          "K14 for m up to 8192: persistent 128-row tiles, cross rows in a "
          "grid-bounded scratch, M panels shared through LDS (CDNA4)",
          pybind11::arg("X"), pybind11::arg("A"), pybind11::arg("s2"),
          pybind11::arg("amp"), pybind11::arg("mv"), pybind11::arg("M"),
          pybind11::arg("kxx"), pybind11::arg("want_var"),
          pybind11::arg("family") = (int)GEOM_FAM_RBF,
          pybind11::arg("max_blocks") = 0);
  mod.def("ppa_predict_wide_supported", &ppa_predict_wide_supported);
  mod.def("greedy_pass1", &greedy_pass1,
          "greedy selection round, pass 1: column c, U[mc], p and the "
          "sums (V c, c.c, c.y) (K15, CDNA4)",
          pybind11::arg("X"), pybind11::arg("xstar"), pybind11::arg("s2"),
          pybind11::arg("amp"), pybind11::arg("y"), pybind11::arg("a"),
          pybind11::arg("a_nn"), pybind11::arg("mc"), pybind11::arg("U"),
          pybind11::arg("V"), pybind11::arg("c"), pybind11::arg("p"),
          pybind11::arg("partials"), pybind11::arg("sums"),
          pybind11::arg("family") = (int)GEOM_FAM_RBF);
  mod.def("greedy_pass2", &greedy_pass2,
          "greedy selection round, pass 2: V[mc], q, mu, the scores and "
          "their argmax (K15, CDNA4)",
          pybind11::arg("c"), pybind11::arg("y"), pybind11::arg("l"),
          pybind11::arg("l_nn"), pybind11::arg("beta_new"),
          pybind11::arg("kxx"), pybind11::arg("sigma2"), pybind11::arg("n"),
          pybind11::arg("mc"), pybind11::arg("V"), pybind11::arg("p"),
          pybind11::arg("q"), pybind11::arg("mu"), pybind11::arg("delta"),
          pybind11::arg("bval"), pybind11::arg("bidx"),
          pybind11::arg("best"));
  mod.def("greedy_supported", &greedy_supported,
          "shapes the greedy kernels take (memory is the caller's check)",
          pybind11::arg("n"), pybind11::arg("m"), pybind11::arg("d"));
  mod.def("greedy_npad", [](int64_t n) { return (int64_t)gr_npad((long)n); },
          "rows of the greedy state: n up to whole blocks");
  mod.def("greedy_blocks",
          [](int64_t n) { return (int64_t)gr_blocks((long)n); });
  mod.def("greedy_state_bytes",
          [](int64_t n, int64_t m) {
            return (int64_t)gr_state_bytes((long)n, (long)m);
          },
          "device bytes of the state of a selection of m among n rows",
          pybind11::arg("n"), pybind11::arg("m"));
  mod.def("kmeans_assign", &kmeans_assign,
          "Lloyd step, part 1: every row's nearest centroid, no [n, m] "
          "array (K16, CDNA4)",
          pybind11::arg("X"), pybind11::arg("centers"), pybind11::arg("c2"),
          pybind11::arg("assign"));
  mod.def("kmeans_accumulate", &kmeans_accumulate,
          "Lloyd step, part 2: fp64 sums and counts per centroid in a fixed "
          "order, no atomics (K16, CDNA4)",
          pybind11::arg("X"), pybind11::arg("assign"),
          pybind11::arg("partials"), pybind11::arg("sums"),
          pybind11::arg("counts"));
  mod.def("kmeans_supported", &kmeans_supported,
          "shapes the k-means kernels take (memory is the caller's check)",
          pybind11::arg("n"), pybind11::arg("m"), pybind11::arg("d"));
  mod.def("kmeans_slice_rows", []() { return (int64_t)KM_SLICE; },
          "rows of one fp32 accumulation of kmeans_accumulate");
  mod.def("kmeans_npad", [](int64_t n) { return (int64_t)km_npad((long)n); },
          "elements of assign: n up to whole row tiles");
  mod.def("kmeans_mpad", [](int64_t m) { return (int64_t)km_mpad((int)m); },
          "elements of c2: m up to whole centroid panels");
  mod.def("kmeans_partial_doubles",
          [](int64_t n, int64_t m, int64_t d) {
            return (int64_t)km_partial_doubles((long)n, (long)m, (long)d);
          },
          "elements of the partials of kmeans_accumulate",
          pybind11::arg("n"), pybind11::arg("m"), pybind11::arg("d"));
  mod.def("syrk_bf16_sync_acc", &syrk_bf16_sync_acc,
          "k-synchronized persistent SYRK for large m (CDNA4)");
  mod.def("syrk_bf16_acc", &syrk_bf16_acc,
          "KK += K K^T of the transposed block KcT [m, c]; bf16 MFMA, "
          "fp32 accumulate (CDNA4)");
  mod.def("colsum_gemv_acc", &colsum_gemv_acc,
          "Ky += Kc^T y, fp64 accumulate (CDNA4)");
}
