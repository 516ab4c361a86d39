"""harness.RGCN on blocks really sampled by RelNeighborSampler, fp32 on the native kernels, against the float64 global-id reference of
tests/_global_ref.py: logits, every parameter gradient and the gradient of the feature table.

The graph is that of tests/_model_cases.py (a hub of 300 in-edges, a node without one, a self-loop, a repeated edge; three edge types),
its in-edges sorted by type.  The fan-outs mix 0, k and -1 in the output layer: [[3, 3, 3], [0, 2, -1]] in model order.  The blocks are
first compared with the restatement of tests/_rel_fanout_ref.py, exactly.  Tolerance: the rgcn tolerance of test_models_global_gpu.py,
FACTOR = 4 times the difference of the reference's own float32 and float64 evaluations (test_models_global_gpu.py:35, imported)."""
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _global_ref as R
import _model_cases as MC
from _full_ref import bucketed
from _rel_fanout_ref import reference_layers, sort_by_type
from test_models_global_gpu import FACTOR

pytestmark = pytest.mark.gpu

FANOUTS = [[3, 3, 3], [0, 2, -1]]
# model -> the sampler's step, which also seeds the parameters and the loss matrix: the first step in 0, 1, 2, ... at which the kink gap
# of the float64 reference on the restatement's blocks is at least 1.5 tau (found on the CPU; the test asks for tau)
# Measured there, gap / tau: rgcn 1.9e-04 / 1.6e-06, rgcn_basis 2.0e-05 / 1.5e-06, the same with and without owner bucketing.
STEPS = {"rgcn": 0, "rgcn_basis": 0}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(None)
def sorted_graph():
    g = MC.graph()
    perm = sort_by_type(g.indptr, g.etype)
    return g._replace(indices=g.indices[perm], w=g.w[perm], etype=g.etype[perm])


def reference_blocks(step, G):
    """The blocks of the case from the restatement, as CPU Block objects in model order (what STEPS was found on)."""
    import torch
    from COALA_GNN.sampler import Block
    g = sorted_graph()
    host = MC.HostGraph(g)
    layers = reference_layers(g.indptr, g.indices, g.etype, g.seeds, list(reversed(FANOUTS)), MC.SAMPLER_SEED, step)
    blocks, dst = [], g.seeds
    for l, (src, ip, loc, eid) in enumerate(layers):
        kw = {}
        if G and l == len(layers) - 1:
            ids, sizes, new_of_old = bucketed(src, G)
            kw = dict(dst_in_src=torch.from_numpy(new_of_old[: len(dst)].astype(np.int32)), dst_nodes=torch.from_numpy(src[: len(dst)].copy()))
            loc, src = new_of_old[loc], ids
        blocks.insert(0, Block(torch.from_numpy(np.ascontiguousarray(src)), None, len(dst), graph=host if l == 0 else None, edata_graph=host,
                               indptr=torch.from_numpy(ip), indices=torch.from_numpy(np.asarray(loc, dtype=np.int32)),
                               eid=torch.from_numpy(eid), **kw))
        dst = layers[l][0]
    return blocks


def evaluation(model_kind, step, blocks, model):
    g = sorted_graph()
    layers = [R.decode(b) for b in blocks]
    return R.Evaluation(model_kind, MC.params_of(model), g.X, MC.loss_matrix(step), layers, {"w": g.w, "etype": g.etype}, heads=MC.HEADS,
                        num_rels=MC.NRELS)


@pytest.fixture(scope="module")
def device_graph(hiplib):
    import torch
    from COALA_GNN.sampler import RelNeighborSampler, sort_csc_by_etype
    g = MC.graph()
    d_ip, d_ix, d_et = (torch.from_numpy(a).cuda() for a in (g.indptr, g.indices, g.etype))
    s_ix, s_et, perm = sort_csc_by_etype(d_ip, d_ix, d_et)
    s = sorted_graph()
    assert np.array_equal(s_ix.cpu().numpy(), s.indices) and np.array_equal(s_et.cpu().numpy(), s.etype)
    dg = RelNeighborSampler.make_graph(d_ip, s_ix, ndata={"labels": torch.from_numpy(g.labels).cuda()},
                                       edata={"etype": s_et, "w": torch.from_numpy(g.w).cuda()[perm]})
    yield dg, torch.from_numpy(g.X).cuda()
    dg.close()


@pytest.mark.parametrize("G", [0, 3])
@pytest.mark.parametrize("kind", ["rgcn", "rgcn_basis"])
def test_rgcn_on_relation_sampled_blocks(device_graph, monkeypatch, kind, G):
    import torch
    from COALA_GNN import sampler as S
    from COALA_GNN.sampler import RelNeighborSampler
    native, real = [], S._RelSumCSR
    monkeypatch.setattr(S, "_RelSumCSR", type("Spy", (), {"apply": staticmethod(lambda *a: (native.append(1), real.apply(*a))[1])}))
    dg, X = device_graph
    g = sorted_graph()
    step = STEPS[kind]
    smp = RelNeighborSampler(FANOUTS, MC.NRELS, seed=MC.SAMPLER_SEED, bucket_by_owner=G)
    input_nodes, _, blocks = smp.sample(dg, torch.from_numpy(g.seeds).cuda(), step=step)
    # the integer part, exact: the blocks are the restatement's, and a row holds min(deg_r, f_r) edges of relation r
    want = reference_blocks(step, G)
    deg_all = np.zeros((MC.N, MC.NRELS), dtype=np.int64)
    np.add.at(deg_all, (np.repeat(np.arange(MC.N), np.diff(g.indptr)), g.etype), 1)
    for b, wb, fan in zip(blocks, want, FANOUTS):
        assert np.array_equal(b.src_nodes.cpu().numpy(), wb.src_nodes.numpy()) and np.array_equal(b.indptr.cpu().numpy(), wb.indptr.numpy())
        assert np.array_equal(b.indices.cpu().numpy(), wb.indices.numpy()) and np.array_equal(b.edata["_ID"].cpu().numpy(), wb.edata["_ID"].numpy())
        assert (b.dst_in_src is None) == (wb.dst_in_src is None) and (b.dst_in_src is None or np.array_equal(b.dst_in_src.cpu().numpy(), wb.dst_in_src.numpy()))
        f = np.array(fan)
        deg = deg_all[b.dstdata["_ID"].cpu().numpy()]
        take = np.where(f == 0, 0, np.where(f < 0, deg, np.minimum(deg, f)))
        assert np.array_equal(b.rel_in_degrees(b.edata["etype"], MC.NRELS).cpu().numpy(), take), "rel_in_degrees != min(deg_r, f_r)"
    assert torch.equal(input_nodes, blocks[0].src_nodes) and (G == 0 or blocks[0].dst_in_src is not None)
    assert np.array_equal(blocks[-1].dstdata["labels"].cpu().numpy().reshape(-1), g.labels[g.seeds])
    model = MC.make_model(kind, len(blocks), step)
    ev = evaluation(kind, step, blocks, model)
    print(f"{kind}-b{G}: kink gap {ev.gap:.3e} tau {ev.tau:.3e}")
    assert ev.gap >= ev.tau, "the inputs sit on a gradient discontinuity: choose another step for this case on the CPU"
    got = MC.run_model(model.cuda(), blocks, X, torch.from_numpy(MC.loss_matrix(step)).cuda())
    assert len(native) == len(blocks), "every layer must have gone through the native relation-typed sum"
    ev.check_kernel(got, f"{kind}-b{G}", FACTOR)


def test_train_synthetic_with_rel_sampler(hiplib):
    """examples/train_synthetic.py --model_type rgcn --sampler rel in a child process with its own time limit: one short epoch, a finite
    loss."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), "--nodes", "60000", "--dim", "64", "--batch_size", "256",
           "--epochs", "1", "--cache_size", "4", "--prefetch", "1", "--model_type", "rgcn", "--num_rels", "4", "--sampler", "rel",
           "--rel_fan_out", "4,3,0,-1;3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    first, last = re.search(r"first loss (\S+)", r.stdout), re.search(r"final loss (\S+)", r.stdout)
    assert first and last and "Test Acc" in r.stdout, r.stdout[-2000:]
    print(f"loss {first.group(1)} -> {last.group(1)}")
    assert math.isfinite(float(first.group(1))) and math.isfinite(float(last.group(1)))
