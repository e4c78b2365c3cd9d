// patch_weights_check -- a host program around ppfw_patch_weights
// (include/ppfitsw.h), built together with psrfits.cpp and psrfits_write.cpp so
// that the host compiler's sanitizers see all of it:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -DPPF_SRC_HASH='"x"' -Iinclude
//       tools/patch_weights_check.cpp pulseportraiture_amd/csrc/psrfits.cpp
//       pulseportraiture_amd/csrc/psrfits_write.cpp -o patch_weights_check
//   patch_weights_check FILE
//
// FILE is a fold-mode PSRFITS file with at least two subints and two
// channels.  It patches two cells, reads them back through the reader, tries
// what must be refused (the file may not change then), restores the two
// cells and checks that the file is byte for byte what it was.  Prints "ok".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ppfits.h"
#include "ppfitsw.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond);   \
      ++failures;                                                   \
    }                                                               \
  } while (0)

std::vector<unsigned char> slurp(const char* path) {
  std::vector<unsigned char> out;
  FILE* fp = fopen(path, "rb");
  if (!fp) return out;
  unsigned char buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) out.insert(out.end(), buf, buf + n);
  fclose(fp);
  return out;
}

bool weights(const char* path, int32_t* nsub, int32_t* nchan, std::vector<double>* w) {
  ppfits_file* f = nullptr;
  if (ppfits_open(path, &f) != PPFITS_OK) {
    fprintf(stderr, "%s: %s\n", path, ppfits_error(f));
    ppfits_close(f);
    return false;
  }
  ppfits_info I;
  bool ok = ppfits_get_info(f, &I) == PPFITS_OK;
  if (ok) {
    *nsub = I.nsub;
    *nchan = I.nchan;
    w->assign((size_t)I.nsub * I.nchan, -1.0);
    ok = ppfits_read_meta(f, nullptr, w->data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr) == PPFITS_OK;
  }
  ppfits_close(f);
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s FILE\n", argv[0]);
    return 2;
  }
  const char* path = argv[1];
  const std::vector<unsigned char> before = slurp(path);
  int32_t nsub = 0, nchan = 0;
  std::vector<double> w0, w1;
  if (!weights(path, &nsub, &nchan, &w0) || nsub < 2 || nchan < 2) {
    fprintf(stderr, "%s: need a fold-mode file of >= 2 subints x 2 channels\n", path);
    return 2;
  }
  char err[256] = "";

  // two cells, one of them the table's last
  const int32_t isub[2] = {0, nsub - 1}, ichan[2] = {1, nchan - 1};
  const double val[2] = {0.0, 0.5};
  CHECK(ppfw_patch_weights(path, 2, isub, ichan, val, err, sizeof err) == PPFITS_OK);
  CHECK(err[0] == '\0');
  CHECK(weights(path, &nsub, &nchan, &w1));
  for (size_t i = 0; i < w1.size(); ++i) {
    double want = w0[i];
    if (i == 1) want = 0.0;
    if (i == w1.size() - 1) want = 0.5;
    CHECK(w1[i] == want);
  }
  const std::vector<unsigned char> patched = slurp(path);
  CHECK(patched.size() == before.size());

  // refused, file untouched: indices outside the table, in any position
  const int32_t bad_sub[2] = {0, nsub}, bad_chan[2] = {0, nchan}, neg[2] = {0, -1};
  const int32_t zero[2] = {0, 0};
  CHECK(ppfw_patch_weights(path, 2, bad_sub, zero, val, err, sizeof err) == PPFITS_ERR_RANGE);
  CHECK(strlen(err) > 0);
  CHECK(ppfw_patch_weights(path, 2, zero, bad_chan, val, err, sizeof err) == PPFITS_ERR_RANGE);
  CHECK(ppfw_patch_weights(path, 2, neg, zero, val, nullptr, 0) == PPFITS_ERR_RANGE);
  CHECK(ppfw_patch_weights(path, 2, zero, neg, val, err, 1) == PPFITS_ERR_RANGE);
  CHECK(ppfw_patch_weights(path, 1, nullptr, zero, val, err, sizeof err) == PPFITS_ERR_MISSING);
  CHECK(ppfw_patch_weights(nullptr, 0, nullptr, nullptr, nullptr, err, sizeof err) ==
        PPFITS_ERR_MISSING);
  CHECK(slurp(path) == patched);
  // nothing to patch is fine, and changes nothing
  CHECK(ppfw_patch_weights(path, 0, nullptr, nullptr, nullptr, err, sizeof err) == PPFITS_OK);
  CHECK(slurp(path) == patched);
  // no such file
  const std::string missing = std::string(path) + ".does-not-exist";
  CHECK(ppfw_patch_weights(missing.c_str(), 2, isub, ichan, val, err, sizeof err) == PPFITS_ERR_IO);

  // the two cells back: the file is what it was
  const double back[2] = {w0[1], w0[w0.size() - 1]};
  CHECK(ppfw_patch_weights(path, 2, isub, ichan, back, err, sizeof err) == PPFITS_OK);
  CHECK(slurp(path) == before);

  if (failures) return 1;
  puts("ok");
  return 0;
}
