// Stand-alone CPU restatement of the local-distortion chain of sflow.hip on the shared arithmetic of sflow_core.h (plain C++,
// no HIP): planes and parameters in; descriptors, the top level's cost volume, the flow and LD out.  tests/test_sflow_cpu.py
// builds it with -fsanitize=address,undefined and holds every output to tests/sflow_model.py byte for byte.
//   sflow_host_check in.bin out.bin
// in.bin : int32 h, w, then the ten int32 fields of dvd_sflow_params in their order, then plane A and plane B, h*w bytes each
// out.bin: descriptors of A on level 0 [h,w,128] u8, the top level's cost volume [h_top,w_top,L_top] u16, the flow [2,h,w]
//          int16, LD as one f64
// stdout : "status h_top w_top L_top"; a refused shape or parameter prints its status (DVD_E_ARG) and writes nothing.
#include "sflow_host_chain.hpp"

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: sflow_host_check in.bin out.bin\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[12];
  if (fread(head, sizeof(int32_t), 12, f) != 12) return 2;
  const int h = head[0], w = head[1];
  dvd_sflow_params pr;
  memcpy(&pr, head + 2, sizeof(pr));
  static_assert(sizeof(dvd_sflow_params) == 10 * sizeof(int32_t), "ten int fields");
  const char* why = check_params(pr);
  if (!why) why = check_shape(h, w, pr);
  if (why) {
    fclose(f);
    fprintf(stderr, "refused: %s\n", why);
    printf("%d 0 0 0\n", DVD_E_ARG);
    return 0;
  }
  const size_t hw = (size_t)h * w;
  Bytes a(hw), b(hw);
  if (fread(a.data(), 1, hw, f) != hw || fread(b.data(), 1, hw, f) != hw) return 2;
  fclose(f);
  const LevelDims dm = level_dims(h, w, pr.levels);
  std::vector<int16_t> flow;
  std::vector<uint16_t> top_cost;
  Bytes da0;
  const double ld = chain(a, b, h, w, pr, flow, &da0, &top_cost);
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 2;
  fwrite(da0.data(), 1, da0.size(), g);
  fwrite(top_cost.data(), sizeof(uint16_t), top_cost.size(), g);
  fwrite(flow.data(), sizeof(int16_t), flow.size(), g);
  fwrite(&ld, sizeof(double), 1, g);
  fclose(g);
  const int wt = level_win(pr, pr.levels - 1);
  printf("0 %d %d %d\n", dm.h[pr.levels - 1], dm.w[pr.levels - 1], (2 * wt + 1) * (2 * wt + 1));
  return 0;
}
