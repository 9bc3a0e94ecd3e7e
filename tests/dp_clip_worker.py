"""Rank program of tests/test_grad_clip_dp_gpu.py (NOT a test module): started by that test module as
`python -m torch.distributed.run --nproc-per-node 2 tests/dp_clip_worker.py <out_dir>` before the pytest process touches the GPU.
Every rank runs three clipped steps (FusedAdam(max_grad_norm=...)) through mer_amd.dp.DataParallelStep on its shard of three global
batches, with the fp32 and with the bf16 gradient exchange, and leaves `clip_rank<r>.pt` in <out_dir> (losses, the published norm /
coefficient of every step, parameters after every step) for the test to compare between the ranks and against one process stepping
on the whole batches; it also records what overlap=True answers with clipping on.  Backend as in tests/dp_worker.py: RCCL with one
GPU per rank, gloo (host-staged sums) with both ranks on cuda:0 on a one-GPU box."""
import os
import sys
import traceback

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "src"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASE = "tiny_ragged"
MAX_GRAD_NORM = 0.01          # far below the gradient norm of the seeded model (about 1): every step clips; the test asserts it
LR, WEIGHT_DECAY = 1e-3, 0.01


def global_batches():
    """Three global batches of the tiny_ragged model (ragged, different shapes)."""
    import synth
    cfg, B, L, lengths, k = synth.CASES[CASE]
    return cfg, [synth.make_inputs(cfg, B, L, lengths, k, seed=11),
                 synth.make_inputs(cfg, 4, 8, [8, 3, 6, 5], k, seed=12),
                 synth.make_inputs(cfg, 6, 12, [12, 2, 9, 12, 5, 7], k, seed=13)]


def shard(batch, rank, world):
    from mer_amd import dp
    mine = dp.shard_dialogues(batch[2].shape[0], rank, world)
    if not mine:
        return [t[:0].contiguous() for t in batch]
    keep = int((~batch[2][mine]).sum(1).max())
    return [t[mine][:, :keep].contiguous() for t in batch]


def main():
    out_dir = sys.argv[1]
    from mer_amd import dp
    import synth
    from mer_amd.model import M2FNet
    from mer_amd.optim import FusedAdam
    world = int(os.environ["WORLD_SIZE"])
    n_gpu = torch.cuda.device_count()
    backend = "nccl" if n_gpu >= world else "gloo"
    os.environ["M2F_DIST_BACKEND"] = backend
    rank, world, local = dp.init_distributed(backend)
    device = torch.device("cuda", local if backend == "nccl" else 0)
    torch.cuda.set_device(device)
    res = {"backend": backend, "world": world, "rank": rank}
    cfg, batches = global_batches()
    shards = [shard(b, rank, world) for b in batches]
    for name, precision, exchange in (("fp32", "fp32", "fp32"), ("bf16", "bf16", "bf16")):
        torch.manual_seed(0)
        m = M2FNet(cfg, precision=precision).to(device).train()
        m.load_state_dict({k: v.to(device) for k, v in synth.make_state_dict(cfg).items()})
        opt = FusedAdam(m, lr=LR, weight_decay=WEIGHT_DECAY, max_grad_norm=MAX_GRAD_NORM)
        step = dp.DataParallelStep(m, opt, n_buckets=3, exchange=exchange, overlap=False)
        losses, params, norms, coefs, fresh = [], [], [], [], []
        for i, sh in enumerate(shards):
            loss = step(*[t.to(device) for t in sh], use_graph=i > 0)
            losses.append(float(loss))
            torch.cuda.synchronize()
            norms.append(opt.grad_norm().detach().cpu().clone())
            coefs.append(opt.clip_coef().detach().cpu().clone())
            fresh.append(m.engine().shadows_fresh())
            params.append(m.flat_parameters().detach().cpu().clone())
        res[name] = {"losses": losses, "params": params, "norms": norms, "coefs": coefs, "fresh": fresh,
                     "exchange": step.reducer.exchange, "g16": m.engine().grad_bf16_buf is not None}
    # overlap=True with clipping: refused on every rank alike, before any launch or collective of the step
    torch.manual_seed(0)
    m = M2FNet(cfg, precision="bf16").to(device).train()
    m.load_state_dict({k: v.to(device) for k, v in synth.make_state_dict(cfg).items()})
    opt = FusedAdam(m, lr=LR, weight_decay=WEIGHT_DECAY, max_grad_norm=MAX_GRAD_NORM)
    step = dp.DataParallelStep(m, opt, n_buckets=3, exchange="bf16", overlap=True)
    try:
        step(*[t.to(device) for t in shards[0]], use_graph=False)
        res["overlap"] = "no error"
    except RuntimeError as e:
        res["overlap"] = str(e)
    torch.save(res, os.path.join(out_dir, f"clip_rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except Exception:                                       # leave the traceback where the test can show it
        with open(os.path.join(sys.argv[1], f"clip_error_rank{os.environ.get('RANK', '0')}.txt"), "w") as f:
            f.write(traceback.format_exc())
        raise
