"""Rank program of tests/test_grad_accumulation_dp_gpu.py (NOT a test module): started by that test module as
`python -m torch.distributed.run --nproc-per-node 2 tests/dp_accum_worker.py <out_dir>` before the pytest process touches the GPU.
Every rank runs groups of two micro-batches through mer_amd.dp.DataParallelStep - sync=False, then sync=True - and leaves
`acc_rank<r>.pt` in <out_dir> (losses, parameters after each group, the shards it ran) for the test to compare against one
process that accumulates all micro-batches of all ranks.  Backend as in tests/dp_worker.py: RCCL with one GPU per rank, gloo
(host-staged sums) with both ranks on cuda:0 on a one-GPU box."""
import os
import sys
import traceback

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "src"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASE = "tiny_ragged"


def global_micro_batches(kind):
    """Two global micro-batches of the tiny_ragged model.  kind "empty": the second holds ONE dialogue (rank 1's shard is empty)."""
    import synth
    cfg, B, L, lengths, k = synth.CASES[CASE]
    first = synth.make_inputs(cfg, B, L, lengths, k, seed=11)
    second = synth.make_inputs(cfg, 1, 7, [7], k, seed=13) if kind == "empty" else synth.make_inputs(cfg, 4, 8, [8, 3, 6, 5], k, seed=12)
    return cfg, [first, second]


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
    for name, precision, exchange, kind in (("fp32", "fp32", "fp32", "full"), ("empty", "fp32", "fp32", "empty"),
                                            ("bf16", "bf16", "bf16", "full")):
        cfg, mbs = global_micro_batches(kind)
        shards = [shard(b, rank, world) for b in mbs]
        torch.manual_seed(0)
        m = M2FNet(cfg, precision=precision).to(device).train()
        m.load_state_dict({k: v.to(device) for k, v in synth.make_state_dict(cfg).items()})
        opt = FusedAdam(m, lr=1e-3, weight_decay=0.01)
        step = dp.DataParallelStep(m, opt, n_buckets=3, exchange=exchange)
        losses, params = [], []
        for g in range(2):                                  # two groups: the first micro-batch of the second one overwrites again
            for j, sh in enumerate(shards):
                loss = step(*[t.to(device) for t in sh], use_graph=g > 0, sync=j == len(shards) - 1)
            losses.append(float(loss))
            torch.cuda.synchronize()
            params.append(m.flat_parameters().detach().cpu().clone())
        res[name] = {"losses": losses, "params": params, "shards": shards, "g16": m.engine().grad_bf16_buf is not None}
    torch.save(res, os.path.join(out_dir, f"acc_rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except Exception:                                       # leave the traceback where the test can show it
        with open(os.path.join(sys.argv[1], f"acc_error_rank{os.environ.get('RANK', '0')}.txt"), "w") as f:
            f.write(traceback.format_exc())
        raise
