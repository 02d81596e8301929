"""Per-launch table of a rocprofv3 kernel trace of tools/fwd_once.py (B = 512), attributed to the plan's launch rows like tools/analyze_trace.py, with the
standard error of each mean and the k_gn_apply pass in front of a conv_gn_upfold launch (profiles/r07/up_fold_gemm_by_shape.txt: the parent's tree against this one).
usage: trace_by_shape.py <rocprofv3 output dir> <repository tree whose libnatinf.so made the trace> <label>"""
import csv, glob, sys, ctypes as C, math, os
from collections import defaultdict
trace_dir, tree, label = sys.argv[1], sys.argv[2], sys.argv[3]
lib = C.CDLL(os.path.join(tree, "naturaldiffusion_amd", "libnatinf.so"))
h = C.c_void_p(); lib.natinf_ncsnpp_create(C.byref(h), 0)
buf = C.create_string_buffer(1 << 16)
lib.natinf_ncsnpp_describe_gemms.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
lib.natinf_ncsnpp_describe_gemms(h, 512, buf, len(buf))
shapes = []
for l in buf.value.decode().strip().split("\n"):
    M, N, K0, K1, taps, batch, k = l.split()
    shapes.append((int(M), int(N), int(K0) + int(K1), int(batch), k))
f = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))[0]
allrows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6      # ms
gem = [i for i, r in enumerate(allrows) if "k_gemm" in r["Kernel_Name"] or "k_conv_gn" in r["Kernel_Name"] or "k_head_conv" in r["Kernel_Name"]]
assert len(gem) % len(shapes) == 0, (len(gem), len(shapes))
nfwd = len(gem) // len(shapes)
skip = 3                                                 # warm-up forwards left out
agg = defaultdict(list); pre = []; fwd = defaultdict(float)
for j, i in enumerate(gem):
    if j // len(shapes) < skip: continue
    s = shapes[j % len(shapes)]
    agg[s].append(dur(allrows[i]))
    if "upfold" in s[4]:
        p = allrows[i - 1]
        assert "k_gn_apply" in p["Kernel_Name"], p["Kernel_Name"]
        pre.append(dur(p))
# device time of every kernel per forward (sum of kernel durations between the first launches of consecutive forwards)
starts = [gem[k * len(shapes)] for k in range(nfwd)] + [len(allrows)]
per_fwd = [sum(dur(r) for r in allrows[starts[k]:starts[k + 1]]) for k in range(skip, nfwd - 1)]
def ms(v): m = sum(v) / len(v); se = math.sqrt(sum((x - m) ** 2 for x in v) / (len(v) - 1) / len(v)) if len(v) > 1 else 0.0; return m, se
print(f"# {label}: {nfwd} forwards traced, the first {skip} left out; ms per launch = mean +- standard error of the mean")
print(f"{'M':>7} {'N':>5} {'K':>5} {'kernel':>22} {'calls':>6} {'ms/call':>8} {'+-se':>7} {'TF/s':>7}")
tot = 0.0
for s, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
    m, se = ms(v); tot += sum(v)
    print(f"{s[0]:7d} {s[1]:5d} {s[2]:5d} {s[4]:>22} {len(v):6d} {m:8.4f} {se:7.4f} {2.0*s[0]*s[1]*s[2]*s[3]/m/1e9:7.1f}")
if pre:
    m, se = ms(pre)
    print(f"k_gn_apply at 16x16 in front of conv_gn_upfold: {len(pre)} calls, {m:.4f} +- {se:.4f} ms")
m, se = ms(per_fwd)
print(f"sum of ALL kernel durations per forward: {m:.3f} +- {se:.3f} ms over {len(per_fwd)} forwards; GEMM-shaped launches {tot / (nfwd - skip):.3f} ms per forward")
