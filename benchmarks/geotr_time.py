#!/usr/bin/env python3
"""Time of the GeoTr init-flow prior (env.use_init_flow; dvd_amd.prestage.GeoTr) per document, alone and in a batch, with
the split over its stages (encoder = fnet on the conv-net executor, transformer = 12 attention layers, upsampling = the
update block + the fused convex upsampling / resize to G) and the achieved TF/s against the f32 matrix peak (every stage
runs in exact f32: v_mfma_f32_32x32x2_f32 GEMMs, f32 FMA attention).
usage: python benchmarks/geotr_time.py [batches=1,32] [grid=64]"""
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dvd_amd import prestage, synth  # noqa: E402

PEAK_F32 = 157.3e12        # MI355X f32 matrix (= vector) peak, spec
BATCHES = [int(b) for b in (sys.argv[1] if len(sys.argv) > 1 else "1,32").split(",")]
G = int(sys.argv[2]) if len(sys.argv) > 2 else 64
T, D = 1296, 256


def conv_flops(P, hw_in):
    """2 * MACs of every conv of a Program (output size from the stride)."""
    sizes, total, conv_i = {0: hw_in}, 0, 0
    for o in P.ops:
        h, w = sizes[o["a"]]
        if o["op"] == prestage.CONV:
            _, cin, cout, ks, _ = P.convs[conv_i]
            conv_i += 1
            if o.get("flag", 0) == 2:
                pad = ks // 2
                h, w = (h + 2 * pad - ks) // 2 + 1, (w + 2 * pad - ks) // 2 + 1
            total += 2 * cout * cin * ks * ks * h * w
        sizes[o["dst"]] = (h, w)
    return total


def transformer_flops():
    per_layer = (2 * T * D * 512 + 2 * T * D * D + 4 * T * T * D + 2 * T * D * D      # self-attention
                 + 3 * 2 * T * D * D + 4 * T * T * D + 2 * T * D * D                  # cross-attention
                 + 2 * 2 * T * D * 2048)                                              # FFN
    return 12 * per_layer, 12 * 2 * 4 * T * T * D


def main():
    m = prestage.GeoTr_Seg_Inf()
    m.msk.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_convnet_state_dict("u2netp", 11).items()})
    m.GeoTr.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_geotr_state_dict(31).items()})
    m.to("cuda").eval()
    geo = m.GeoTr
    f_enc = conv_flops(geo._program, (288, 288))
    f_tr, f_attn = transformer_flops()
    f_up = conv_flops(geo._upd_program, (36, 36))
    print(f"GFLOP per document: encoder {f_enc / 1e9:.1f}, transformer {f_tr / 1e9:.1f} (attention cores {f_attn / 1e9:.1f}), "
          f"update block {f_up / 1e9:.2f}")
    print(f"device {torch.cuda.get_device_name()}, f32 matrix peak {PEAK_F32 / 1e12:.1f} TF/s")
    for n in BATCHES:
        y = torch.stack([torch.from_numpy(synth.smooth_image(f"gt/{i}", 288, 288, 1)) for i in range(n)]).cuda()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

        def one(record=False):
            nets, w = geo._weights(n)
            if record:
                ev[0].record()
            fmap = nets[0].run(y)[0]
            if record:
                ev[1].record()
            # the transformer + the update block through stages(); fnet runs again inside, so time it separately
            st = geo.stages(y)
            if record:
                ev[2].record()
            geo.upsample(st["dflow"], st["mask"], G, False)
            if record:
                ev[3].record()
            return fmap
        for _ in range(2):
            one()
        torch.cuda.synchronize()
        walls = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            geo.run(y, G, False)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        one(True)
        torch.cuda.synchronize()
        t_enc = ev[0].elapsed_time(ev[1])
        t_rest = ev[1].elapsed_time(ev[2]) - t_enc          # stages() = fnet + transformer + update convs
        t_up = ev[2].elapsed_time(ev[3])
        ms = sorted(walls)[2]
        tf = lambda f, t: f * n / (t * 1e-3) / 1e12  # noqa: E731
        print(f"batch {n:3d}: {ms / n:8.3f} ms per document (wall {ms:.2f} ms per pass) | encoder {t_enc / n:.3f} ms "
              f"{tf(f_enc, t_enc):.1f} TF/s | transformer + update convs {t_rest / n:.3f} ms {tf(f_tr + f_up, t_rest):.1f} TF/s "
              f"({tf(f_tr + f_up, t_rest) * 1e12 / PEAK_F32:.2f} of peak) | convex upsampling {t_up / n * 1e3:.1f} us | "
              f"all {tf(f_enc + f_tr + f_up, ms):.1f} TF/s")


if __name__ == "__main__":
    main()
