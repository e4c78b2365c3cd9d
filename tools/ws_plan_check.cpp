// ws_plan_check.cpp -- the workspace plans of libppfit's eight chunked sites
// (ppfit_wsplan.hpp), checked against the arithmetic they replaced, as a
// stand-alone host program (no GPU, no HIP):
//
//   g++ -std=c++17 -O1 -Wall -Werror -Ipulseportraiture_amd/csrc tools/ws_plan_check.cpp
//       -o ws_plan_check
//   ./ws_plan_check
//
// Each site's arrays are declared here the way its host file declares them
// (ppfit_capi_*.hip), at small shapes.  kCases holds, as literal numbers from
// the hand-written formulas the planner replaced, the chunk, every offset and
// the total of: 11 items under a limit of 1 byte (chunk 1), under 3 and under
// 4 - 1/divisor times the site's divisor (chunk 3 from both ends, which pins
// the divisor to the byte) and under the default 32 GiB (chunk 11); and, for
// the sites capped at 65535 items, 65538 items under the default limit.  The
// plan's total is the old one rounded up to a multiple of 256, and so is the
// Gaussian fit's join flag behind its arrays.  Exit status 0 and "ok": every
// case agrees.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ppfit_wsplan.hpp"

using namespace ppf;

namespace {

// sizes the library takes from its kernels' headers
constexpr size_t kDouble2 = 16, kSolveState = 576, kPcaState = 24, kGaussFitState = 32;
constexpr int kMT = 32, kSwtGrid = 30, kGfLmDoubles = 20520, kGramTile = 64, kGramSlab = 256;
constexpr int kFsSlice = 32;

struct Case {
  const char* site;
  int v1, v2;  // fit: taylor, wide; swt: L; gauss: njoin (-1: none), fit
  long long nitem, limit, chunk;
  unsigned long long total;
  size_t noff;
  unsigned long long off[10];
};

const Case kCases[] = {
    {"fit", 0, 0, 11, 1LL, 1, 10752ULL, 10, {0ULL, 6144ULL, 6912ULL, 7680ULL, 7936ULL, 8192ULL, 8960ULL, 10240ULL, 10752ULL, 10752ULL}},
    {"fit", 0, 0, 11, 33600LL, 3, 30720ULL, 10, {0ULL, 18432ULL, 20736ULL, 23040ULL, 23296ULL, 23552ULL, 25344ULL, 29184ULL, 30720ULL, 30720ULL}},
    {"fit", 0, 0, 11, 44799LL, 3, 30720ULL, 10, {0ULL, 18432ULL, 20736ULL, 23040ULL, 23296ULL, 23552ULL, 25344ULL, 29184ULL, 30720ULL, 30720ULL}},
    {"fit", 0, 0, 11, 34359738368LL, 11, 112128ULL, 10, {0ULL, 67584ULL, 76032ULL, 84480ULL, 85248ULL, 86016ULL, 92416ULL, 106496ULL, 112128ULL, 112128ULL}},
    {"fit", 0, 1, 11, 1LL, 1, 11264ULL, 10, {0ULL, 6144ULL, 6912ULL, 7680ULL, 7936ULL, 8192ULL, 8960ULL, 10240ULL, 10752ULL, 10752ULL}},
    {"fit", 0, 1, 11, 35136LL, 3, 32256ULL, 10, {0ULL, 18432ULL, 20736ULL, 23040ULL, 23296ULL, 23552ULL, 25344ULL, 29184ULL, 30720ULL, 30720ULL}},
    {"fit", 0, 1, 11, 46847LL, 3, 32256ULL, 10, {0ULL, 18432ULL, 20736ULL, 23040ULL, 23296ULL, 23552ULL, 25344ULL, 29184ULL, 30720ULL, 30720ULL}},
    {"fit", 0, 1, 11, 34359738368LL, 11, 117760ULL, 10, {0ULL, 67584ULL, 76032ULL, 84480ULL, 85248ULL, 86016ULL, 92416ULL, 106496ULL, 112128ULL, 112128ULL}},
    {"fit", 1, 0, 11, 1LL, 1, 14848ULL, 10, {0ULL, 6144ULL, 6912ULL, 7680ULL, 7936ULL, 8192ULL, 8960ULL, 10240ULL, 10752ULL, 14848ULL}},
    {"fit", 1, 0, 11, 45888LL, 3, 43008ULL, 10, {0ULL, 18432ULL, 20736ULL, 23040ULL, 23296ULL, 23552ULL, 25344ULL, 29184ULL, 30720ULL, 43008ULL}},
    {"fit", 1, 0, 11, 61183LL, 3, 43008ULL, 10, {0ULL, 18432ULL, 20736ULL, 23040ULL, 23296ULL, 23552ULL, 25344ULL, 29184ULL, 30720ULL, 43008ULL}},
    {"fit", 1, 0, 11, 34359738368LL, 11, 157184ULL, 10, {0ULL, 67584ULL, 76032ULL, 84480ULL, 85248ULL, 86016ULL, 92416ULL, 106496ULL, 112128ULL, 157184ULL}},
    {"fit", 1, 1, 11, 1LL, 1, 15360ULL, 10, {0ULL, 6144ULL, 6912ULL, 7680ULL, 7936ULL, 8192ULL, 8960ULL, 10240ULL, 10752ULL, 14848ULL}},
    {"fit", 1, 1, 11, 47424LL, 3, 44544ULL, 10, {0ULL, 18432ULL, 20736ULL, 23040ULL, 23296ULL, 23552ULL, 25344ULL, 29184ULL, 30720ULL, 43008ULL}},
    {"fit", 1, 1, 11, 63231LL, 3, 44544ULL, 10, {0ULL, 18432ULL, 20736ULL, 23040ULL, 23296ULL, 23552ULL, 25344ULL, 29184ULL, 30720ULL, 43008ULL}},
    {"fit", 1, 1, 11, 34359738368LL, 11, 162816ULL, 10, {0ULL, 67584ULL, 76032ULL, 84480ULL, 85248ULL, 86016ULL, 92416ULL, 106496ULL, 112128ULL, 157184ULL}},
    {"phase_tau", 0, 0, 11, 1LL, 1, 528ULL, 1, {0ULL}},
    {"phase_tau", 0, 0, 11, 1584LL, 3, 1584ULL, 1, {0ULL}},
    {"phase_tau", 0, 0, 11, 2111LL, 3, 1584ULL, 1, {0ULL}},
    {"phase_tau", 0, 0, 11, 34359738368LL, 11, 5808ULL, 1, {0ULL}},
    {"fscrunch", 0, 0, 11, 1LL, 1, 1808ULL, 2, {0ULL, 1280ULL}},
    {"fscrunch", 0, 0, 11, 6288LL, 3, 4912ULL, 2, {0ULL, 3328ULL}},
    {"fscrunch", 0, 0, 11, 8383LL, 3, 4912ULL, 2, {0ULL, 3328ULL}},
    {"fscrunch", 0, 0, 11, 34359738368LL, 11, 17584ULL, 2, {0ULL, 11776ULL}},
    {"pca", 0, 0, 11, 1LL, 1, 2568ULL, 4, {0ULL, 2048ULL, 2304ULL, 2560ULL}},
    {"pca", 0, 0, 11, 9408LL, 3, 6680ULL, 4, {0ULL, 6144ULL, 6400ULL, 6656ULL}},
    {"pca", 0, 0, 11, 12543LL, 3, 6680ULL, 4, {0ULL, 6144ULL, 6400ULL, 6656ULL}},
    {"pca", 0, 0, 11, 34359738368LL, 11, 23640ULL, 4, {0ULL, 22528ULL, 23040ULL, 23552ULL}},
    {"pca", 0, 0, 65538, 34359738368LL, 65535, 138409976ULL, 4, {0ULL, 134215680ULL, 136312832ULL, 137885696ULL}},
    {"gram", 0, 0, 11, 1LL, 1, 66824ULL, 7, {0ULL, 32768ULL, 65536ULL, 65792ULL, 66304ULL, 66560ULL, 66816ULL}},
    {"gram", 0, 0, 11, 204504LL, 3, 198936ULL, 7, {0ULL, 98304ULL, 196608ULL, 196864ULL, 198400ULL, 198656ULL, 198912ULL}},
    {"gram", 0, 0, 11, 272671LL, 3, 198936ULL, 7, {0ULL, 98304ULL, 196608ULL, 196864ULL, 198400ULL, 198656ULL, 198912ULL}},
    {"gram", 0, 0, 11, 34359738368LL, 11, 727896ULL, 7, {0ULL, 360448ULL, 720896ULL, 721408ULL, 727040ULL, 727296ULL, 727808ULL}},
    {"gram", 0, 0, 65538, 34359738368LL, 65535, 4333174264ULL, 7, {0ULL, 2147450880ULL, 4294901760ULL, 4296998912ULL, 4330552832ULL, 4331077120ULL, 4332649984ULL}},
    {"swt", 1, 0, 11, 1LL, 1, 2312ULL, 7, {0ULL, 1024ULL, 1280ULL, 1536ULL, 1792ULL, 2048ULL, 2304ULL}},
    {"swt", 1, 0, 11, 4104LL, 3, 4888ULL, 7, {0ULL, 3072ULL, 3328ULL, 3584ULL, 3840ULL, 4608ULL, 4864ULL}},
    {"swt", 1, 0, 11, 5471LL, 3, 4888ULL, 7, {0ULL, 3072ULL, 3328ULL, 3584ULL, 3840ULL, 4608ULL, 4864ULL}},
    {"swt", 1, 0, 11, 34359738368LL, 11, 15192ULL, 7, {0ULL, 11264ULL, 11520ULL, 11776ULL, 12032ULL, 14848ULL, 15104ULL}},
    {"swt", 1, 0, 65538, 34359738368LL, 65535, 85195768ULL, 7, {0ULL, 67107840ULL, 67632128ULL, 67894272ULL, 68418560ULL, 84147200ULL, 84671488ULL}},
    {"swt", 5, 0, 11, 1LL, 1, 7464ULL, 7, {0ULL, 5120ULL, 5376ULL, 5632ULL, 5888ULL, 7168ULL, 7424ULL}},
    {"swt", 5, 0, 11, 19560LL, 3, 20344ULL, 7, {0ULL, 15360ULL, 15616ULL, 15872ULL, 16128ULL, 19968ULL, 20224ULL}},
    {"swt", 5, 0, 11, 26079LL, 3, 20344ULL, 7, {0ULL, 15360ULL, 15616ULL, 15872ULL, 16128ULL, 19968ULL, 20224ULL}},
    {"swt", 5, 0, 11, 34359738368LL, 11, 71608ULL, 7, {0ULL, 56320ULL, 56832ULL, 57088ULL, 57344ULL, 70656ULL, 71168ULL}},
    {"swt", 5, 0, 65538, 34359738368LL, 65535, 422832088ULL, 7, {0ULL, 335539200ULL, 338160640ULL, 338422784ULL, 338947072ULL, 417589248ULL, 420210688ULL}},
    {"gauss", -1, 0, 11, 1LL, 1, 34080ULL, 10, {0ULL, 14336ULL, 29184ULL, 31488ULL, 32000ULL, 32256ULL, 33792ULL, 34048ULL, 34048ULL, 34080ULL}},
    {"gauss", -1, 0, 11, 112296LL, 3, 100704ULL, 10, {0ULL, 43008ULL, 87552ULL, 93952ULL, 95488ULL, 95744ULL, 100096ULL, 100608ULL, 100608ULL, 100704ULL}},
    {"gauss", -1, 0, 11, 149727LL, 3, 100704ULL, 10, {0ULL, 43008ULL, 87552ULL, 93952ULL, 95488ULL, 95744ULL, 100096ULL, 100608ULL, 100608ULL, 100704ULL}},
    {"gauss", -1, 0, 11, 34359738368LL, 11, 367456ULL, 10, {0ULL, 157696ULL, 320512ULL, 343808ULL, 349184ULL, 349696ULL, 365568ULL, 367104ULL, 367104ULL, 367456ULL}},
    {"gauss", -1, 0, 65538, 34359738368LL, 65535, 2184675552ULL, 10, {0ULL, 939509760ULL, 1908379392ULL, 2046789376ULL, 2078246400ULL, 2080343552ULL, 2174714112ULL, 2182578432ULL, 2182578432ULL, 2184675552ULL}},
    {"gauss", -1, 1, 11, 1LL, 1, 198432ULL, 10, {0ULL, 14336ULL, 29184ULL, 31488ULL, 32000ULL, 32256ULL, 33792ULL, 34048ULL, 198400ULL, 198432ULL}},
    {"gauss", -1, 1, 11, 604776LL, 3, 593248ULL, 10, {0ULL, 43008ULL, 87552ULL, 93952ULL, 95488ULL, 95744ULL, 100096ULL, 100608ULL, 593152ULL, 593248ULL}},
    {"gauss", -1, 1, 11, 806367LL, 3, 593248ULL, 10, {0ULL, 43008ULL, 87552ULL, 93952ULL, 95488ULL, 95744ULL, 100096ULL, 100608ULL, 593152ULL, 593248ULL}},
    {"gauss", -1, 1, 11, 34359738368LL, 11, 2173280ULL, 10, {0ULL, 157696ULL, 320512ULL, 343808ULL, 349184ULL, 349696ULL, 365568ULL, 367104ULL, 2172928ULL, 2173280ULL}},
    {"gauss", -1, 1, 65538, 34359738368LL, 65535, 12942901216ULL, 10, {0ULL, 939509760ULL, 1908379392ULL, 2046789376ULL, 2078246400ULL, 2080343552ULL, 2174714112ULL, 2182578432ULL, 12940804096ULL, 12942901216ULL}},
    {"gauss", 2, 0, 11, 1LL, 1, 34848ULL, 10, {0ULL, 14336ULL, 29184ULL, 31488ULL, 32256ULL, 32512ULL, 34304ULL, 34560ULL, 34560ULL, 34592ULL}},
    {"gauss", 2, 0, 11, 113736LL, 3, 102496ULL, 10, {0ULL, 43008ULL, 87552ULL, 93952ULL, 96000ULL, 96256ULL, 101632ULL, 102144ULL, 102144ULL, 102240ULL}},
    {"gauss", 2, 0, 11, 151647LL, 3, 102496ULL, 10, {0ULL, 43008ULL, 87552ULL, 93952ULL, 96000ULL, 96256ULL, 101632ULL, 102144ULL, 102144ULL, 102240ULL}},
    {"gauss", 2, 0, 11, 34359738368LL, 11, 373088ULL, 10, {0ULL, 157696ULL, 320512ULL, 343808ULL, 350720ULL, 351232ULL, 370688ULL, 372480ULL, 372480ULL, 372832ULL}},
    {"gauss", 2, 0, 65538, 34359738368LL, 65535, 2216132576ULL, 10, {0ULL, 939509760ULL, 1908379392ULL, 2046789376ULL, 2086634752ULL, 2088731904ULL, 2204073728ULL, 2214035200ULL, 2214035200ULL, 2216132320ULL}},
    {"gauss", 2, 1, 11, 1LL, 1, 199200ULL, 10, {0ULL, 14336ULL, 29184ULL, 31488ULL, 32256ULL, 32512ULL, 34304ULL, 34560ULL, 198912ULL, 198944ULL}},
    {"gauss", 2, 1, 11, 606216LL, 3, 595040ULL, 10, {0ULL, 43008ULL, 87552ULL, 93952ULL, 96000ULL, 96256ULL, 101632ULL, 102144ULL, 594688ULL, 594784ULL}},
    {"gauss", 2, 1, 11, 808287LL, 3, 595040ULL, 10, {0ULL, 43008ULL, 87552ULL, 93952ULL, 96000ULL, 96256ULL, 101632ULL, 102144ULL, 594688ULL, 594784ULL}},
    {"gauss", 2, 1, 11, 34359738368LL, 11, 2178912ULL, 10, {0ULL, 157696ULL, 320512ULL, 343808ULL, 350720ULL, 351232ULL, 370688ULL, 372480ULL, 2178304ULL, 2178656ULL}},
    {"gauss", 2, 1, 65538, 34359738368LL, 65535, 12974358240ULL, 10, {0ULL, 939509760ULL, 1908379392ULL, 2046789376ULL, 2086634752ULL, 2088731904ULL, 2204073728ULL, 2214035200ULL, 12972260864ULL, 12974357984ULL}},
    {"bank", 0, 0, 11, 1LL, 1, 928ULL, 2, {0ULL, 768ULL}},
    {"bank", 0, 0, 11, 3600LL, 3, 2272ULL, 2, {0ULL, 1792ULL}},
    {"bank", 0, 0, 11, 4799LL, 3, 2272ULL, 2, {0ULL, 1792ULL}},
    {"bank", 0, 0, 11, 34359738368LL, 11, 7648ULL, 2, {0ULL, 5888ULL}},
    {"bank", 0, 0, 65538, 34359738368LL, 65535, 45088096ULL, 2, {0ULL, 34602496ULL}},
};

size_t meta_lds(int nchan) { return align256((size_t)nchan * (5 * sizeof(double) + sizeof(int))); }
size_t xspec_dyn_lds(int nchan) {
  return (size_t)nchan * kDouble2 + (((size_t)nchan + 15) & ~(size_t)15);
}

// ppfit_capi_fit.hip, FitWorkspace
void plan_fit(WsPlan& ws, int nchan, int NHP, bool taylor, bool wide, int64_t n, int64_t limit) {
  const size_t bR = (size_t)NHP * kDouble2, bC = (size_t)nchan * sizeof(double);
  ws.array((size_t)nchan * NHP * kDouble2);
  ws.array(bR);
  ws.array(bR);
  ws.array(bC);
  ws.array(bC);
  ws.array(kSolveState);
  ws.array((size_t)2 * nchan * 10 * sizeof(double));
  ws.array((size_t)nchan * 8 * sizeof(double));
  ws.array(taylor ? (size_t)2 * nchan * kMT * sizeof(double) : 0);
  ws.array(wide ? align256(std::max(meta_lds(nchan), xspec_dyn_lds(nchan))) : 0);
  ws.lay_out(n, limit, 1024);
}

// ppfit_capi_rows.hip, ppf_phase_tau_batch
void plan_phase_tau(WsPlan& ws, int nbin, int64_t n, int64_t limit) {
  ws.array(((size_t)nbin / 2 + 1) * kDouble2);
  ws.lay_out(n, limit, 0);
}

// ppfit_capi_rows.hip, ppf_rotate_fscrunch
void plan_fscrunch(WsPlan& ws, int nchan, int nbin, int64_t n, int64_t limit) {
  const int NH = nbin / 2 + 1, nslice = (nchan + kFsSlice - 1) / kFsSlice;
  ws.array((size_t)nslice * NH * kDouble2);
  ws.array((size_t)NH * kDouble2);
  ws.lay_out(n, limit, 512, (int64_t)0x7fffffff / nslice);
}

// ppfit_capi_pca.hip, ppf_pca_portraits
void plan_pca(WsPlan& ws, int nchan, int nbin, int ncomp, int64_t n, int64_t limit) {
  const int m = nchan;
  ws.array((size_t)m * nbin * sizeof(double));
  ws.array((size_t)m * sizeof(double));
  ws.array(kPcaState);
  ws.array((size_t)ncomp * sizeof(int));
  ws.lay_out(n, limit, 1024, 65535);
}

// ppfit_capi_pca.hip, ppf_pca_gram_portraits
void plan_gram(WsPlan& ws, int nchan, int nbin, int ncomp, int64_t n, int64_t limit) {
  const int m = nbin, ntile = (nbin + kGramTile - 1) / kGramTile;
  const int npair = ntile * (ntile + 1) / 2, nslab = (nchan + kGramSlab - 1) / kGramSlab;
  ws.array((size_t)m * nbin * sizeof(double));
  ws.array((size_t)nslab * npair * kGramTile * kGramTile * sizeof(double));
  ws.array((size_t)nchan * sizeof(double));
  ws.array((size_t)m * sizeof(double));
  ws.array(sizeof(double));
  ws.array(kPcaState);
  ws.array((size_t)ncomp * sizeof(int));
  ws.lay_out(n, limit, 2048, 65535);
}

// ppfit_capi_swt.hip, swt_chunks
void plan_swt(WsPlan& ws, int nbin, int L, int64_t n, int64_t limit) {
  ws.array((size_t)L * 2 * nbin * sizeof(double));
  ws.array((size_t)L * sizeof(double));
  ws.array(sizeof(int));
  ws.array(sizeof(double));
  ws.array((size_t)L * kSwtGrid * sizeof(double));
  ws.array((size_t)L * sizeof(double));
  ws.array((size_t)L * sizeof(double));
  ws.lay_out(n, limit, 64 + 4, 65535);
}

// ppfit_capi_gauss.hip, gauss_plan; *oBad: the join flag's offset
void plan_gauss(WsPlan& ws, int nchan, int nbin, int ngauss, int njoin, bool fit, int64_t n,
                int64_t limit, size_t* oBad) {
  const bool join = njoin >= 0;
  const int npar = 3 + 6 * ngauss + (join ? 2 * njoin : 0), KT = 1 + 3 * ngauss;
  const int KB = KT + 2 + (join ? 1 : 0), npairs = KB * (KB + 1) / 2, NH = nbin / 2 + 1;
  const size_t rows = (size_t)nchan;
  ws.array(rows * KT * nbin * sizeof(double));
  ws.array(rows * KT * NH * kDouble2);
  ws.array(rows * NH * kDouble2);
  ws.array(rows * npar * sizeof(double));
  ws.array(rows * sizeof(double));
  ws.array(rows * npairs * sizeof(double));
  ws.array((size_t)npar * sizeof(double));
  ws.array(fit ? (size_t)kGfLmDoubles * sizeof(double) : 0);
  ws.array(kGaussFitState);
  ws.lay_out(n, limit, 4096, 65535);
  *oBad = ws.total;
  if (join) ws.total += 256;
}

// ppfit_capi_gauss.hip, ppf_gauss_bank
void plan_bank(WsPlan& ws, int nbin, int nwid, int64_t n, int64_t limit) {
  ws.array(((size_t)nbin / 2 + 1) * kDouble2);
  ws.array((size_t)nwid * 4 * sizeof(double));
  ws.lay_out(n, limit, 512, 65535);
}

int nbad = 0;

#define CHECK(c, cond)                                                                    \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      fprintf(stderr, "%s (%d, %d) nitem %lld limit %lld: %s failed\n", (c).site, (c).v1, \
              (c).v2, (c).nitem, (c).limit, #cond);                                       \
      ++nbad;                                                                             \
    }                                                                                     \
  } while (0)

void check(const Case& c) {
  WsPlan ws;
  size_t oBad = 0;
  const bool gauss = !strcmp(c.site, "gauss");
  if (!strcmp(c.site, "fit")) plan_fit(ws, 8, 48, c.v1 != 0, c.v2 != 0, c.nitem, c.limit);
  else if (!strcmp(c.site, "phase_tau")) plan_phase_tau(ws, 64, c.nitem, c.limit);
  else if (!strcmp(c.site, "fscrunch")) plan_fscrunch(ws, 40, 64, c.nitem, c.limit);
  else if (!strcmp(c.site, "pca")) plan_pca(ws, 4, 64, 2, c.nitem, c.limit);
  else if (!strcmp(c.site, "gram")) plan_gram(ws, 4, 64, 2, c.nitem, c.limit);
  else if (!strcmp(c.site, "swt")) plan_swt(ws, 64, c.v1, c.nitem, c.limit);
  else if (gauss) plan_gauss(ws, 4, 64, 2, c.v1, c.v2 != 0, c.nitem, c.limit, &oBad);
  else if (!strcmp(c.site, "bank")) plan_bank(ws, 64, 5, c.nitem, c.limit);
  else CHECK(c, !"a known site");
  CHECK(c, ws.chunk == c.chunk);
  // (the Gaussian fit's last entry is the join flag, behind the arrays)
  const size_t narray = gauss ? c.noff - 1 : c.noff;
  CHECK(c, (size_t)ws.narray == narray);
  for (size_t a = 0; a < narray && a < (size_t)ws.narray; ++a) CHECK(c, ws.off[a] == c.off[a]);
  CHECK(c, ws.total == align256(c.total));
  if (gauss) CHECK(c, oBad == align256(c.off[c.noff - 1]));
  // no array reaches into the next one or past the total
  for (int a = 0; a < ws.narray; ++a) {
    const size_t end = ws.off[a] + (size_t)ws.chunk * ws.per[a];
    CHECK(c, end <= (a + 1 < ws.narray ? ws.off[a + 1] : ws.total));
  }
}

}  // namespace

int main() {
  int n3 = 0, ncap = 0;
  for (const Case& c : kCases) {
    check(c);
    n3 += c.chunk == 3;
    ncap += c.chunk == 65535;
  }
  // the table itself: two chunk-3 cases per variant, one capped case per capped variant
  if (n3 != 30 || ncap != 9) {
    fprintf(stderr, "table: %d chunk-3 and %d capped cases\n", n3, ncap);
    ++nbad;
  }
  // at() walks an array by its own bytes per item
  WsPlan ws;
  const int a0 = ws.array(24), a1 = ws.array(8);
  ws.lay_out(11, 1 << 20, 0);
  static char buf[1024];
  ws.base = buf;
  if (ws.at<char>(a0, 2) != buf + 48 || ws.at<char>(a1, 3) != buf + 512 + 24) {
    fprintf(stderr, "at(): wrong address\n");
    ++nbad;
  }
  if (nbad) return 1;
  printf("ok\n");
  return 0;
}
