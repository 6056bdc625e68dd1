// correction_coded_rate_harness.cpp — vnr::correction_coded_record_bits (csrc/correction_coded_format.cpp), the closed form of a coded
// record's length, held to what the writer beside it really writes; for tests/test_correction_coded_rate_host.py, which builds it
// with csrc/correction_coded_format.cpp, csrc/correction_packed_format.cpp and csrc/correction_format.cpp under
// -fsanitize=address,undefined (a stand-alone program).
//
//   harness CORPUS      CORPUS: fixed-width ("VNRCORR1") corrections, each behind a u32 with its length
// For every correction one line "blob <n_flagged>", then for every flagged cell one line "<words> <bits of record 0> <of record 1> ...":
// the bits by the closed form from the magnitudes of the fixed-width codes, the words their sum filled up to 64.  The words must be
// what the cell table of correction_coded_from_fixed says the writer wrote: exit code 4 otherwise.
#include "correction_coded_format.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<char> all((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  size_t at = 0;
  while (at + 4 <= all.size()) {
    uint32_t len;
    std::memcpy(&len, &all[at], 4);
    at += 4;
    if (at + len > all.size()) return 3;
    std::vector<uint8_t> in(all.begin() + (long)at, all.begin() + (long)(at + len));   // exactly `len` bytes on the heap
    at += len;
    const vnr::CorrectionData d = vnr::correction_parse(in.data(), in.size());
    const std::vector<uint8_t> coded = vnr::correction_coded_from_fixed(d.h, d.cells, d.payload);
    std::printf("blob %zu\n", d.cells.size());
    uint64_t offset = 0;
    for (size_t i = 0; i < d.cells.size(); ++i) {
      const uint32_t width = d.cells[i].width;
      const uint64_t voxels = vnr::correction_cell_voxels(d.h.dims, d.cells[i].cell), groups = vnr::correction_cell_groups(voxels);
      std::vector<uint32_t> bits(groups);
      uint64_t total = 0;
      for (uint64_t k = 0; k < groups; ++k) {
        uint64_t m[vnr::kCorrectionGroup] = {};
        const uint64_t lanes = std::min<uint64_t>(vnr::kCorrectionGroup, voxels - vnr::kCorrectionGroup * k);
        for (uint64_t l = 0; l < lanes; ++l) {
          uint64_t u = 0;
          std::memcpy(&u, d.payload.data() + offset + (vnr::kCorrectionGroup * k + l) * width, width);
          if (d.h.kind != vnr::kCorrectionVerbatim) {
            const uint32_t shift = 64 - 8 * width;
            const int64_t q = (int64_t)(u << shift) >> shift;   // sign-extended
            u = q < 0 ? 0 - (uint64_t)q : (uint64_t)q;
          }
          m[l] = u;
        }
        bits[k] = vnr::correction_coded_record_bits(m, d.h.kind);
        total += bits[k];
      }
      offset += vnr::correction_padded_bytes(voxels, width);
      uint32_t written;
      std::memcpy(&written, coded.data() + 4 * i, 4);
      if (written != (total + 63) / 64) {
        std::fprintf(stderr, "cell %u: the writer wrote %u words, the closed form gives %llu\n", d.cells[i].cell, written, (unsigned long long)((total + 63) / 64));
        return 4;
      }
      std::printf("%llu", (unsigned long long)((total + 63) / 64));
      for (uint32_t b : bits) std::printf(" %u", b);
      std::printf("\n");
    }
  }
  return 0;
}
