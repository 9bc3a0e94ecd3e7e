"""Record the bits of the streaming attention kernels (csrc/attention_stream.hip, csrc/attention_stream_chunk.hip) into
tests/golden/stream_kernel_bits.npz: for every case below the output tensor of the dense launch and a SHA-256 of the K and of the V
cache bytes after it.  tests/test_stream_kernel_bits_gpu.py regenerates the inputs with the functions of this file and holds the dense
and the paged form to these bits, so a change of the kernels that moves both forms together (another summation order inside the
tolerance, say) still shows.  The fixture is recorded ONCE, on the commit before such a change; a run that differs from it is a finding
about the kernels, not a reason to record again.  The tool itself refuses to write unless the paged form gives the dense form's bits.

Inputs come from numpy.random.RandomState(seed), whose stream is the same in every numpy version.  A cache holds random rows where an
utterance is cached and NaN everywhere else (so a read of a dead row shows in the output); pad columns of the live rows are zeros.
The paged form gets the same rows scattered into NaN pools through a page table that is a non-identity permutation (a slot's ids
descend, the slots interleave); its pools are compared after gathering them back through the table.

    python tools/record_stream_bits.py [--out FILE]           (on the GPU; writes the fixture)"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "stream_kernel_bits.npz")
S, H, R = 3, 2, 16
DEV = "cuda"


def cases():
    """-> list of dicts: kind 'step' | 'chunk', bf16, hd, C, ring, lens [S], and active [S] (step) or T, new [S] (chunk)"""
    out = []
    for bf16 in (False, True):
        for hd in (20, 128):          # 5 chunks of 4 floats / 3 of 8 bf16 per row: idle lanes, pad columns; 128: 32 lanes per row
            base = {"bf16": bf16, "hd": hd}
            out.append(dict(base, kind="step", name="plain", C=40, ring=False, lens=[0, 17, 39], active=[1, 1, 1]))
            out.append(dict(base, kind="step", name="plain_inactive", C=40, ring=False, lens=[0, 17, 39], active=[1, 0, 1]))
            out.append(dict(base, kind="step", name="ring", C=40, ring=True, lens=[39, 40, 95], active=[1, 1, 1]))
            # the history crosses the 64-row block and the page boundaries
            out.append(dict(base, kind="chunk", name="plain", C=80, ring=False, lens=[0, 62, 75], T=5, new=[0, 3, 5]))
            # more new rows than the ring holds; the dead row
            out.append(dict(base, kind="chunk", name="ring", C=8, ring=True, lens=[0, 8, 21], T=16, new=[16, 9, 1]))
    for i, c in enumerate(out):
        c["seed"] = 1000 + i
        c["key"] = "{kind}_{p}_hd{hd}_{name}".format(p="bf16" if c["bf16"] else "fp32", **c)
    return out


def inputs(case):
    """-> (q, k, v [rows, H*hd] fp32, kcache, vcache [S, H, C, pad(hd)] fp32 / bf16) on the device, from RandomState(case['seed'])"""
    rs = np.random.RandomState(case["seed"])
    hd, C, bf16 = case["hd"], case["C"], case["bf16"]
    rows = S * case.get("T", 1)
    q, k, v = (torch.from_numpy(rs.standard_normal((rows, H * hd)).astype(np.float32)).to(DEV) for _ in range(3))
    hdp = (hd + 7) // 8 * 8 if bf16 else (hd + 3) // 4 * 4
    caches = []
    for _ in range(2):
        live = torch.from_numpy(rs.standard_normal((S, H, C, hd)).astype(np.float32))
        c = torch.full((S, H, C, hdp), float("nan"))
        for s, n in enumerate(case["lens"]):
            c[s, :, :min(n, C), :hd] = live[s, :, :min(n, C)]
            c[s, :, :min(n, C), hd:] = 0.0
        caches.append(c.to(torch.bfloat16 if bf16 else torch.float32).to(DEV))
    return q, k, v, caches[0], caches[1]


def page_table(C):
    """-> int32 [S, ceil(C / R)] on the host: entry (s, e) = (tw - 1 - e) * S + (S - 1 - s), a permutation of 0 .. S*tw - 1"""
    tw = -(-C // R)
    t = torch.tensor([[(tw - 1 - e) * S + (S - 1 - s) for e in range(tw)] for s in range(S)], dtype=torch.int32)
    assert sorted(t.flatten().tolist()) == list(range(S * tw)) and t.flatten().tolist() != list(range(S * tw))
    return t


def to_pool(cache, table):
    """the dense cache's rows into a NaN pool [S*tw, H, R, hdp] through the table (the last page of a slot: partly filled)"""
    C = cache.shape[2]
    pool = torch.full((table.numel(), H, R, cache.shape[3]), float("nan"), dtype=cache.dtype, device=cache.device)
    for s in range(S):
        for e in range(table.shape[1]):
            n = min((e + 1) * R, C) - e * R
            pool[int(table[s, e]), :, :n] = cache[s, :, e * R: e * R + n]
    return pool


def from_pool(pool, table, C):
    cache = torch.empty((S, H, C, pool.shape[3]), dtype=pool.dtype, device=pool.device)
    for s in range(S):
        for e in range(table.shape[1]):
            n = min((e + 1) * R, C) - e * R
            cache[s, :, e * R: e * R + n] = pool[int(table[s, e]), :, :n]
    return cache


def sha(t):
    """SHA-256 of a tensor's bytes -> uint8 [32]"""
    raw = t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy().tobytes()
    return np.frombuffer(hashlib.sha256(raw).digest(), dtype=np.uint8)


def run(case, paged):
    """One launch of the case's kernel -> (out fp32 ndarray, sha(K cache after), sha(V cache after)); paged: through pools"""
    from mer_amd import functional as F
    q, k, v, kc, vc = inputs(case)
    C, ring, bf16 = case["C"], case["ring"], case["bf16"]
    lengths = torch.tensor(case["lens"], dtype=torch.int32, device=DEV)
    if case["kind"] == "step":
        second = torch.tensor(case["active"], dtype=torch.uint8, device=DEV)
    else:
        second = torch.tensor(case["new"], dtype=torch.int32, device=DEV)
    if paged:
        host = page_table(C)
        table = host.to(DEV)
        kp, vp = to_pool(kc, host), to_pool(vc, host)
        if case["kind"] == "step":
            out = F.attention_stream_paged(q, k, v, kp, vp, table, lengths, second, H, C, ring=ring, bf16=bf16)
        else:
            out = F.attention_stream_chunk_paged(q, k, v, kp, vp, table, lengths, second, H, case["T"], C, ring=ring, bf16=bf16)
        kc, vc = from_pool(kp, host, C), from_pool(vp, host, C)
    elif case["kind"] == "step":
        out = F.attention_stream(q, k, v, kc, vc, lengths, second, H, ring=ring, bf16=bf16)
    else:
        out = F.attention_stream_chunk(q, k, v, kc, vc, lengths, second, H, case["T"], ring=ring, bf16=bf16)
    return out.cpu().numpy(), sha(kc), sha(vc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    import mer_amd  # noqa: F401
    fx = {}
    for case in cases():
        out, ks, vs = run(case, paged=False)
        pout, pks, pvs = run(case, paged=True)
        same = out.tobytes() == pout.tobytes() and ks.tobytes() == pks.tobytes() and vs.tobytes() == pvs.tobytes()
        assert same, "the paged form does not give the dense form's bits: " + case["key"]
        assert np.isfinite(out).all(), "a dead row was read: " + case["key"]
        fx[case["key"] + "/out"], fx[case["key"] + "/k_sha256"], fx[case["key"] + "/v_sha256"] = out, ks, vs
        print(case["key"], out.shape, ks[:4].tobytes().hex(), vs[:4].tobytes().hex(), flush=True)
    np.savez_compressed(args.out, **fx)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
