// tests/test_correction_coded_host.py builds this with csrc/correction_coded_format.cpp, csrc/correction_packed_format.cpp and
// csrc/correction_format.cpp under -fsanitize=address,undefined and feeds it a corpus of coded corrections, valid and damaged: every
// record through the coded reader, and whatever parses through the transcoders (coded -> packed, which the packed reader must take;
// packed -> coded and fixed-width -> coded, which must give the payload back) and through the coded writer back to the same bytes.
// A heap overrun or undefined arithmetic aborts the process; the test sees the exit code.
#include "correction_coded_format.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <vector>

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<char> all((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  size_t at = 0, n_ok = 0, n_err = 0;
  while (at + 4 <= all.size()) {
    uint32_t len;
    std::memcpy(&len, &all[at], 4);
    at += 4;
    if (at + len > all.size()) return 3;
    // a copy of exactly `len` bytes on the heap: one byte beyond it is a sanitizer report
    std::vector<uint8_t> in(all.begin() + (long)at, all.begin() + (long)(at + len));
    at += len;
    vnr::CorrectionCoded c;
    try {
      c = vnr::correction_coded_parse(in.data(), in.size());
    } catch (const std::runtime_error&) {
      ++n_err;
      continue;
    }
    // what the reader let through must transcode into a packed payload the packed reader takes, come back from it and from the
    // fixed-width payload as the same coded payload, and write back to the bytes it came from
    const std::vector<uint8_t> packed = vnr::correction_coded_to_packed(c.h, c.cells, c.payload, c.group_nbits);
    const std::vector<uint8_t> packed_bytes = vnr::correction_packed_write(c.h, c.cells, packed);
    const vnr::CorrectionPacked p = vnr::correction_packed_parse(packed_bytes.data(), packed_bytes.size());
    if (p.payload != packed) { std::fprintf(stderr, "packed round trip differs\n"); return 4; }
    if (vnr::correction_coded_from_packed(c.h, c.cells, packed) != c.payload) { std::fprintf(stderr, "packed -> coded differs\n"); return 4; }
    if (vnr::correction_coded_from_fixed(c.h, c.cells, vnr::correction_unpack(c.h, c.cells, packed)) != c.payload) { std::fprintf(stderr, "fixed -> coded differs\n"); return 4; }
    if (vnr::correction_coded_write(c.h, c.cells, c.payload) != in) { std::fprintf(stderr, "round trip differs\n"); return 4; }
    // the parse's group table alone gives the index of the planes the device decode writes: the one of the transcoded payload
    const vnr::CorrectionPlaneIndex ix = vnr::correction_plane_index_of_table(c.h, c.cells, c.group_nbits.data(), c.group_nbits.size());
    const vnr::CorrectionPlaneIndex whole = vnr::correction_plane_index(c.h, c.cells, packed);
    const std::vector<vnr::CorrectionCellLayout> layout = vnr::correction_cell_layout(c.h, c.cells);
    if (ix.cell_group0 != whole.cell_group0 || ix.cell_word0 != whole.cell_word0 || ix.group_word != whole.group_word || ix.n_words != whole.n_words ||
        layout.size() != c.cells.size() || (!layout.empty() && layout.back().group0 + layout.back().groups != c.group_nbits.size())) {
      std::fprintf(stderr, "layout or index differs\n");
      return 4;
    }
    ++n_ok;
  }
  std::printf("%zu parsed, %zu refused\n", n_ok, n_err);
  return 0;
}
