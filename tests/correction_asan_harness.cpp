// tests/test_error_bound_ref_host.py builds this with csrc/correction_format.cpp under -fsanitize=address,undefined and feeds it a
// corpus of serialised corrections, valid and damaged: every record through the reader, and whatever parses through the writer and
// back to the same bytes.  A heap overrun or undefined arithmetic in the reader aborts the process; the test sees the exit code.
#include "correction_format.h"
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
    try {
      const vnr::CorrectionData c = vnr::correction_parse(in.data(), in.size());
      uint64_t sum = 0;
      for (const vnr::CorrectionCellEntry& e : c.cells) sum += vnr::correction_padded_bytes(vnr::correction_cell_voxels(c.h.dims, e.cell), e.width);
      if (sum != c.payload.size()) { std::fprintf(stderr, "payload size differs\n"); return 4; }
      if (vnr::correction_write(c) != in) { std::fprintf(stderr, "round trip differs\n"); return 4; }
      ++n_ok;
    } catch (const std::exception&) {
      ++n_err;
    }
  }
  std::printf("%zu parsed, %zu refused\n", n_ok, n_err);
  return 0;
}
