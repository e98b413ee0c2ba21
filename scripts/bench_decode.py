"""Times Ocr48Engine.decode at one page (B = 1): 32 lines = 160 beam rows, 32 steps, EOS suppressed; 5 warm-up + 60 timed calls, each
synchronised.  usage: bench_decode.py [TREE_ROOT [LABEL]] — TREE_ROOT: the checkout whose package is measured (default: this one), so that
one copy of the script can time two trees alternately.  Prints one JSON line (milliseconds, and a sha256 over the result tensors)."""
import hashlib, json, os, sys, time
root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, root)
os.chdir(root)
import numpy as np, torch
from manga_image_translator_amd import ocr48, ocr_schema, synth
dev = torch.device("cuda:0")
D = 6004
eng = ocr48.Ocr48Engine(synth.synth_state_dict(ocr_schema.ocr48_schema(D)), D, device=dev)
rng = np.random.default_rng(0)
crops = [rng.integers(0, 256, size=(48, int(rng.integers(180, 600)), 3), dtype=np.uint8) for _ in range(32)]
mks, mvs, lens = [], [], []
for indices, ws, region in eng.make_chunks(crops):
    mk, mv, kl, _ = eng.encode(torch.from_numpy(region).to(dev), ws)
    mks.append(mk.clone()); mvs.append(mv.clone()); lens.append(kl.clone())
Lmax = max(m.shape[2] for m in mks)
pad = lambda m: m if m.shape[2] == Lmax else torch.cat([m, m.new_zeros(5, m.shape[1], Lmax - m.shape[2], 320)], 2)
mem_k, mem_v, klen = torch.cat([pad(m) for m in mks], 1).contiguous(), torch.cat([pad(m) for m in mvs], 1).contiguous(), torch.cat(lens)
assert mem_k.shape[1] == 32
for _ in range(5):
    o = eng.decode(mem_k, mem_v, klen, max_seq_length=32, suppress_eos=True)
torch.cuda.synchronize()
ts = []
for _ in range(60):
    t = time.perf_counter()
    o = eng.decode(mem_k, mem_v, klen, max_seq_length=32, suppress_eos=True)
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t) * 1e3)
ts.sort()
h = hashlib.sha256()
for k in ("tokens", "length", "prob", "colors"):
    h.update(o[k].cpu().numpy().tobytes())
print(json.dumps({"tree": sys.argv[2] if len(sys.argv) > 2 else root, "steps_run": int(o["steps_run"]), "median_ms": round(ts[len(ts) // 2], 4),
                  "min_ms": round(ts[0], 4), "p90_ms": round(ts[54], 4), "sha256": h.hexdigest()}))
