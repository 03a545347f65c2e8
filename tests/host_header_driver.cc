// Driver of tests/test_host_cpu.py::test_level_host_header_alone: the stepper's host half
// (gym-comm_amd/csrc/oc_level_host.h) compiled on its own by the host compiler, under the address
// and undefined-behaviour sanitizers.
//   host_header_driver BLOB WITH_GEOMETRY   BLOB = a level blob (include/oc_level.h), raw int32 words
// prints the text oc_level_spec_source gives for that blob and builds the level's table image.
#include "../gym-comm_amd/csrc/oc_level_host.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::vector<int32_t> blob;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  for (int32_t w; fread(&w, sizeof(w), 1, f) == 1;) blob.push_back(w);
  fclose(f);
  LevelHdr h;
  RunCfg run;
  int32_t slot[OC_MAX_SUBTASKS], goal_index[OC_MAX_SUBTASKS];
  const char *msg = build_header(blob.data(), (int32_t)blob.size(), h, run, slot, goal_index);
  std::vector<uint8_t> img;
  if (!msg) msg = build_tables(blob.data(), h, img);
  if (msg) {
    fprintf(stderr, "%s\n", msg);
    return 1;
  }
  const LevelHdr out = argv[2][0] == '1' ? h : structure_of(h);
  std::vector<char> text(1 << 16);
  const int n = spec_header_text(out, text.data(), (int)text.size());
  if (n >= (int)text.size()) return 3;
  fwrite(text.data(), 1, (size_t)n, stdout);
  return 0;
}
