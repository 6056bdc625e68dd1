// tests/test_correction_pack_host.py builds this with csrc/correction_packed_format.cpp and csrc/correction_format.cpp under
// -fsanitize=address,undefined and feeds it a corpus of packed corrections, valid and damaged: every record through the packed reader,
// and whatever parses through the host unpack (whose result the fixed-width writer and reader must take) and through the packed
// writer back to the same bytes.  A heap overrun or undefined arithmetic aborts the process; the test sees the exit code.
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
    vnr::CorrectionPacked p;
    try {
      p = vnr::correction_packed_parse(in.data(), in.size());
    } catch (const std::runtime_error&) {
      ++n_err;
      continue;
    }
    // what the reader let through must unpack, into a payload the fixed-width form takes, and write back to the bytes it came from
    vnr::CorrectionData v1{p.h, p.cells, vnr::correction_unpack(p.h, p.cells, p.payload)};
    if (v1.payload.size() != vnr::correction_fixed_payload_bytes(p.h, p.cells)) { std::fprintf(stderr, "unpacked size differs\n"); return 4; }
    const std::vector<uint8_t> fixed = vnr::correction_write(v1);
    if (vnr::correction_parse(fixed.data(), fixed.size()).payload != v1.payload) { std::fprintf(stderr, "fixed-width round trip differs\n"); return 4; }
    if (vnr::correction_packed_write(p.h, p.cells, p.payload) != in) { std::fprintf(stderr, "round trip differs\n"); return 4; }
    // the one layout walk and the index from the group table alone: their ends are the sizes of both payloads, and the index of the
    // whole payload is the same index
    const std::vector<vnr::CorrectionCellLayout> layout = vnr::correction_cell_layout(p.h, p.cells);
    const uint64_t n_groups = vnr::correction_n_groups(p.h, p.cells);
    const vnr::CorrectionPlaneIndex ix = vnr::correction_plane_index_of_table(p.h, p.cells, p.payload.data(), n_groups);
    const vnr::CorrectionPlaneIndex whole = vnr::correction_plane_index(p.h, p.cells, p.payload);
    bool same = layout.size() == p.cells.size() && ix.cell_group0 == whole.cell_group0 && ix.cell_word0 == whole.cell_word0 && ix.group_word == whole.group_word &&
                p.payload.size() == vnr::correction_group_table_bytes(n_groups) + 8 * ix.n_words;
    for (size_t i = 0; same && i < layout.size(); ++i) {
      const uint64_t next_codes = i + 1 < layout.size() ? layout[i + 1].codes : v1.payload.size(), next_group = i + 1 < layout.size() ? layout[i + 1].group0 : n_groups;
      same = layout[i].group0 == ix.cell_group0[i] && layout[i].group0 + layout[i].groups == next_group &&
             layout[i].codes + vnr::correction_padded_bytes(layout[i].voxels, p.cells[i].width) == next_codes;
    }
    if (!same) { std::fprintf(stderr, "layout or index differs\n"); return 4; }
    ++n_ok;
  }
  std::printf("%zu parsed, %zu refused\n", n_ok, n_err);
  return 0;
}
