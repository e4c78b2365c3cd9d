// ppfw_check.cpp -- drive the PSRFITS writer (include/ppfitsw.h) and read the
// file back with the reader (include/ppfits.h), as a stand-alone program for
// sanitizer builds of the host code:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude tools/ppfw_check.cpp pulseportraiture_amd/csrc/psrfits.cpp
//       pulseportraiture_amd/csrc/psrfits_write.cpp -o ppfw_check
//   ./ppfw_check ppfw_check.fits
//
// Exit status 0 and "ok": every array came back as written.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ppfits.h"
#include "ppfitsw.h"

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static int run(const char* path, int nsub, int npol, int nchan, int nbin) {
  ppfw_desc d;
  memset(&d, 0, sizeof d);
  d.npol = npol;
  d.nchan = nchan;
  d.nbin = nbin;
  d.dedispersed = 1;
  d.stt_imjd = 57300;
  d.stt_smjd = 43200;
  d.stt_offs = 0.25;
  d.obsfreq = 1500.0;
  d.obsbw = 800.0;
  d.dm = 34.56789;
  snprintf(d.telescope, sizeof d.telescope, "GBT");
  memset(d.source, 'J', sizeof d.source);  // a field with no terminator
  snprintf(d.pol_type, sizeof d.pol_type, npol == 4 ? "IQUV" : "AA+BB");
  snprintf(d.ra, sizeof d.ra, "12:34:00.0");
  snprintf(d.dec, sizeof d.dec, "+56:78:00.0");
  const size_t pc = (size_t)npol * nchan, ns = pc * nbin;
  std::vector<int16_t> raw(nsub * ns);
  std::vector<double> scl(nsub * pc), offs(nsub * pc), freqs((size_t)nsub * nchan),
      wts((size_t)nsub * nchan), tsub(nsub), osub(nsub), per(nsub), pa(nsub);
  for (size_t i = 0; i < raw.size(); ++i) raw[i] = (int16_t)((i * 7919u) % 65535u - 32767);
  for (size_t i = 0; i < scl.size(); ++i) { scl[i] = 0.5f + (float)i; offs[i] = -0.25f * (float)i; }
  for (size_t i = 0; i < freqs.size(); ++i) { freqs[i] = 1100.0 + 0.1 * (double)i; wts[i] = (double)(i % 2); }
  for (int i = 0; i < nsub; ++i) { tsub[i] = 10.0; osub[i] = 5.0 + 10.0 * i; per[i] = 0.003 + 1e-9 * i; pa[i] = 0.5f * i; }

  ppfw_file* w = nullptr;
  CHECK(ppfw_create(path, &d, "PSR J1234+5678\r\nF0 345.678\n\nDM 34.56789", &w) == PPFITS_OK);
  const int n0 = nsub / 2;  // two chunks (the first may be empty)
  CHECK(ppfw_write_subints(w, 0, n0, raw.data(), scl.data(), offs.data(), freqs.data(), wts.data(),
                           tsub.data(), osub.data(), per.data(), pa.data()) == PPFITS_OK);
  CHECK(ppfw_write_subints(w, n0 + 1, 1, raw.data(), scl.data(), offs.data(), freqs.data(),
                           wts.data(), tsub.data(), osub.data(), per.data(), nullptr) ==
        PPFITS_ERR_RANGE);
  CHECK(strstr(ppfw_error(w), "in order") != nullptr);
  CHECK(ppfw_close(w) == PPFITS_ERR_RANGE);  // the first error is the file's status

  CHECK(ppfw_create(path, &d, nullptr, &w) == PPFITS_OK);
  CHECK(ppfw_write_subints(w, 0, n0, raw.data(), scl.data(), offs.data(), freqs.data(), wts.data(),
                           tsub.data(), osub.data(), per.data(), pa.data()) == PPFITS_OK);
  CHECK(ppfw_write_subints(w, n0, nsub - n0, raw.data() + n0 * ns, scl.data() + n0 * pc,
                           offs.data() + n0 * pc, freqs.data() + (size_t)n0 * nchan,
                           wts.data() + (size_t)n0 * nchan, tsub.data() + n0, osub.data() + n0,
                           per.data() + n0, pa.data() + n0) == PPFITS_OK);
  CHECK(ppfw_close(w) == PPFITS_OK);

  ppfits_file* f = nullptr;
  CHECK(ppfits_open(path, &f) == PPFITS_OK);
  ppfits_info I;
  CHECK(ppfits_get_info(f, &I) == PPFITS_OK);
  CHECK(I.nsub == nsub && I.npol == npol && I.nchan == nchan && I.nbin == nbin);
  CHECK(I.raw_type == PPFITS_RAW_I16 && I.dedispersed == 1 && I.dm == 34.56789);
  CHECK(strlen(I.source) == 31);
  std::vector<int16_t> raw2(raw.size());
  std::vector<double> scl2(scl.size()), offs2(offs.size()), freqs2(freqs.size()), wts2(wts.size()),
      tsub2(nsub), osub2(nsub), per2(nsub), pa2(nsub);
  CHECK(ppfits_read_meta(f, freqs2.data(), wts2.data(), offs2.data(), scl2.data(), tsub2.data(),
                         osub2.data(), per2.data(), pa2.data()) == PPFITS_OK);
  CHECK(ppfits_read_raw(f, 0, nsub, raw2.data()) == PPFITS_OK);
  CHECK(raw2 == raw && scl2 == scl && offs2 == offs && freqs2 == freqs && wts2 == wts);
  CHECK(tsub2 == tsub && osub2 == osub && per2 == per && pa2 == pa);
  ppfits_close(f);
  return 0;
}

int main(int argc, char** argv) {
  const char* path = argc > 1 ? argv[1] : "ppfw_check.fits";
  if (run(path, 3, 1, 5, 64) || run(path, 2, 4, 3, 100) || run(path, 1, 1, 1, 16)) return 1;
  ppfw_file* w = nullptr;
  ppfw_desc bad;
  memset(&bad, 0, sizeof bad);
  if (ppfw_create(path, &bad, nullptr, &w) != PPFITS_ERR_FORMAT || ppfw_close(w) != PPFITS_ERR_FORMAT)
    return 1;
  if (ppfw_create("/nonexistent-dir/x.fits", &bad, nullptr, &w) == PPFITS_OK) return 1;
  ppfw_close(w);
  remove(path);
  puts("ok");
  return 0;
}
