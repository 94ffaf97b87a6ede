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
  int h, w;
  dvd_sflow_params pr;
  Bytes a, b;
  const int rc = read_pair(argv[1], h, w, pr, a, b);
  if (rc == DVD_E_ARG) printf("%d 0 0 0\n", DVD_E_ARG);
  if (rc) return rc == DVD_E_ARG ? 0 : rc;
  const LevelDims dm = level_dims(h, w, pr.levels);
  std::vector<int16_t> flow;
  std::vector<uint16_t> top_cost;
  Bytes da0;
  const double ld = chain(a, b, h, w, pr, flow, &da0, &top_cost);
  Bytes out = da0;
  append(out, top_cost.data(), top_cost.size() * sizeof(uint16_t));
  append(out, flow.data(), flow.size() * sizeof(int16_t));
  append(out, &ld, sizeof(double));
  if (!write_all(argv[2], out.data(), out.size())) return 2;
  const int wt = level_win(pr, pr.levels - 1);
  printf("0 %d %d %d\n", dm.h[pr.levels - 1], dm.w[pr.levels - 1], (2 * wt + 1) * (2 * wt + 1));
  return 0;
}
