"""Two (or more) ranks on ONE GPU with gloo: the overlapped, bucketed data-parallel backward must deliver exactly the mean
of the ranks' local gradients.  Each rank first runs fwd+bwd WITHOUT the reducer (its local gradient), the locals are
all-gathered, then the same step runs with the reducer attached (buckets launched from the second stream while backward
is still running).  The engine pre-divides by the world size inside its 1/grad_scale factor (a power of two here), so the
expected buffer is sum_r local_r / world bit for bit.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 tools/dp_check.py [dense|weight80]
"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.distributed as dist
from modelcompression_amd import nets, dp, YOLOV2_VOC_CFG
from modelcompression_amd.synthetic import init_synthetic, synthetic_batch

wl = sys.argv[1] if len(sys.argv) > 1 else "dense"
os.environ["LOCAL_RANK"] = "0"
rank, world = dp.init_from_env("gloo")
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
model = nets.Darknet(YOLOV2_VOC_CFG)
init_synthetic(model, seed=0)
model.to(dev).train()
masks = None
if wl == "weight80":
    from modelcompression_amd.pruning.weightPruning.methods import weight_prune
    masks = weight_prune(model, 80.0)
    dp.broadcast_masks(masks, src=0)
    model.set_masks(masks)
B = 8
x = synthetic_batch(B, 416, 416, seed=rank, device=dev)


def step():
    for p in model.parameters():
        p.grad = None
    out = model(x)
    out.float().mean().backward()
    torch.cuda.synchronize()
    return model._last_flat_grad.clone()


local = step()
again = step()
assert torch.equal(local, again), "the local step is not reproducible"
gathered = [torch.empty_like(local) for _ in range(world)]
dist.all_gather(gathered, local)
expect = torch.zeros_like(local)
for g in gathered:
    expect += g / world                      # power-of-two world: exact
reducer = dp.attach(model, dp.GradReducer(bucket_elems=2 << 20), masks=masks)     # small buckets: many launches mid-backward
got = step()
ok = torch.equal(got, expect)
diff = float((got - expect).abs().max())
line = "rank %d: %s transport, %d collectives, max |dp - mean of locals| = %.3e -> %s\n" % (
    rank, "packed" if masks is not None else "dense", reducer.collectives, diff, "OK" if ok else "MISMATCH")
# the ranks share the launcher's stdout: one write per line (print() issues the text and the newline separately when stdout
# is unbuffered, and the other rank's line can land between them)
sys.stdout.flush()
os.write(sys.stdout.fileno(), line.encode())
t = torch.tensor([1 if ok else 0])
dist.all_reduce(t, op=dist.ReduceOp.MIN)
dist.destroy_process_group()
sys.exit(0 if int(t.item()) == 1 else 1)
