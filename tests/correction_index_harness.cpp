// tests/test_correction_index_host.py builds this with csrc/correction_packed_format.cpp and csrc/correction_format.cpp under
// -fsanitize=address,undefined and runs it on files that each hold one packed correction.  A file goes through the packed reader
// first: what that refuses never reaches correction_plane_index ("refused" is printed instead).  For what parses, the index is
// printed as tests/correction_index_ref.py index_text() writes it, and every code is gathered from the planes through the index
// and compared with the host unpack.  A heap overrun or undefined arithmetic aborts the process; the test sees the exit code.
#include "correction_packed_format.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <vector>

int main(int argc, char** argv)
{
  for (int a = 1; a < argc; ++a) {
    std::ifstream f(argv[a], std::ios::binary);
    const std::vector<char> all((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    // a copy of exactly that many bytes on the heap: one byte beyond it is a sanitizer report
    const std::vector<uint8_t> in(all.begin(), all.end());
    std::printf("file %d\n", a - 1);
    vnr::CorrectionPacked p;
    try {
      p = vnr::correction_packed_parse(in.data(), in.size());
    } catch (const std::runtime_error&) {
      std::printf("refused\n");
      continue;
    }
    const vnr::CorrectionPlaneIndex ix = vnr::correction_plane_index(p.h, p.cells, p.payload);
    std::printf("cells %zu groups %zu words %llu\n", ix.cell_group0.size(), ix.group_word.size(), (unsigned long long)ix.n_words);
    for (size_t i = 0; i < ix.cell_group0.size(); ++i) std::printf("c %llu %llu\n", (unsigned long long)ix.cell_group0[i], (unsigned long long)ix.cell_word0[i]);
    for (uint16_t w : ix.group_word) std::printf("g %u\n", (unsigned)w);
    // every code through the index against the host unpack
    const std::vector<uint8_t> fixed = vnr::correction_unpack(p.h, p.cells, p.payload);
    const uint8_t* table = p.payload.data();
    const uint8_t* planes = table + vnr::correction_group_table_bytes(ix.group_word.size());
    uint64_t offset = 0;
    for (size_t i = 0; i < p.cells.size(); ++i) {
      const uint64_t voxels = vnr::correction_cell_voxels(p.h.dims, p.cells[i].cell);
      const uint32_t width = p.cells[i].width;
      for (uint64_t li = 0; li < voxels; ++li) {
        const uint64_t group = ix.cell_group0[i] + li / 64, word0 = ix.cell_word0[i] + ix.group_word[group];
        uint64_t z = 0;
        for (uint32_t b = 0; b < table[group]; ++b) {
          uint64_t w;
          std::memcpy(&w, planes + 8 * (word0 + b), 8);
          z |= ((w >> (li % 64)) & 1) << b;
        }
        const uint64_t code = p.h.kind == vnr::kCorrectionVerbatim ? z : (z >> 1) ^ (0 - (z & 1));
        if (std::memcmp(&code, fixed.data() + offset + li * width, width) != 0) {
          std::fprintf(stderr, "file %d: code %llu of cell %zu differs from the unpack\n", a - 1, (unsigned long long)li, i);
          return 4;
        }
      }
      offset += vnr::correction_padded_bytes(voxels, width);
    }
  }
  return 0;
}
