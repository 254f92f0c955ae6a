"""Time the GRU recurrence variants (ou_gru_desc.flags) at score-network
shape (H = 256, T = 801) for a few batch sizes; prints us per time step.

GRU_FLAGS: the variants, the first one the reference of identical= (default:
1 the straight-line step loop, 513 the earlier loop (bit9), then older
variants); GRU_B: the batch sizes; GRU_REPS: passes over the flag list,
alternating the variants in one process on one library (a summary line per
variant follows: median and spread (max - min) of its passes' medians)."""
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from open_universe_amd import _lib as L
from open_universe_amd import engine as E
from open_universe_amd.configs import get_config
from open_universe_amd.networks.universe import UniverseGAN
from open_universe_amd.utils.synthetic import synth_state_dict


def main():
    dev = "cuda:0"
    cfg = get_config("pp16")
    m = UniverseGAN(**{k: v for k, v in cfg.items() if k != "_target_"})
    m.load_state_dict(synth_state_dict([(k, v.shape) for k, v in m.state_dict().items()]), strict=False)
    m = m.to(dev).eval()
    eng = m._get_engine()
    T = int(os.environ.get("GRU_T", "801"))
    stream = torch.cuda.current_stream().cuda_stream
    gw = eng.s_gru
    reps = int(os.environ.get("GRU_REPS", "1"))
    for B in [int(b) for b in os.environ.get("GRU_B", "1,4,8").split(",")]:
        x = E.Act(torch.randn(B, 512, T, device=dev) * 0.5)
        gi, y = E.new_act(B, 1536, T, dev), E.new_act(B, 512, T, dev)
        gran = torch.zeros(L.load().ou_gru_workspace_bytes(256, B) // 8, dtype=torch.int64, device=dev)
        ref = None
        flag_list = [int(f) for f in os.environ.get("GRU_FLAGS", "1,513,5,7,9,11,21,25").split(",")]
        meds = {f: [] for f in flag_list}
        for flags in flag_list * reps:
            E.GRU_FLAGS = flags
            prog = L.Program()
            E.rec_gru(prog, gw, 0, x, gi, y, gran, eng.status)
            prog.run(stream)
            torch.cuda.synchronize()
            ms = []
            for _ in range(5):
                t = prog.profile(stream)
                ms.append(t[1])
            out = y.t.clone()
            if ref is None:
                ref = out
            ok = torch.equal(out, ref) and int(eng.status.max()) == 0
            eng.status.zero_()
            meds[flags].append(1000 * sorted(ms)[2] / T)
            print(f"B={B} flags={flags}: {1000 * min(ms) / T:.4f} us/step "
                  f"(median {1000 * sorted(ms)[2] / T:.4f}) identical={ok}", flush=True)
            if os.environ.get("OUHIP_LIB", "").endswith("_diag.so"):
                # phase stamps (OU_GRU_STAMPS build): cycles per step per workgroup
                st = gran[B * 4 * 256 + B * 256 // 4:].view(-1, 8).cpu()
                rows = [r for r in st.tolist() if r[5] > 0]
                names = (("poll", "lds+bar1", "dot", "gate+store", "bar2") if flags & 32 else
                         ("poll", "fma", "reduce", "gate+store", "local_l2x"))
                for w, r in enumerate(rows[:4]):
                    print("   wg%d " % w + " ".join(f"{n}={r[i] / r[5]:.0f}" for i, n in enumerate(names[:4])) + f" {names[4]}={r[4]}",
                          f"total={sum(r[:5]) / r[5]:.0f} cyc/step", flush=True)
        if reps > 1:
            for f, m in meds.items():
                print(f"B={B} flags={f}: {reps} passes, median {sorted(m)[len(m) // 2]:.4f} us/step, "
                      f"spread {max(m) - min(m):.4f}", flush=True)


if __name__ == "__main__":
    main()
