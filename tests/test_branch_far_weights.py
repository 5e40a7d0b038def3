"""The shared-phase branch operators (`parseq_op_attn_fused` variant 1, `parseq_op_mlp_variant` variant 11) take their two weight matrices as
two caller tensors, but the kernels address both through one buffer descriptor with 32-bit offsets.  Two blocks of a caching allocator can lie
more than 4 GiB apart — whether they do depends on everything the process allocated before — and the operators then answered `invalid
argument`.  They stage such a pair side by side now; the result is bit for bit the one with neighbouring weights."""
import pytest
import torch

from gpu_util import DEV, native

pytestmark = pytest.mark.gpu

FAR = (4 << 30) + (64 << 20)      # bytes between the two matrices: past what a 32-bit offset reaches


def _gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _far_apart(a, b):
    """Copies of the bf16 matrices `a` and `b` as views of ONE allocation, FAR bytes apart (the allocation is returned to keep it alive)."""
    span = torch.empty(FAR + b.numel() * 2, dtype=torch.uint8, device=DEV)
    va = span[:a.numel() * 2].view(torch.bfloat16).view(a.shape)
    vb = span[FAR:FAR + b.numel() * 2].view(torch.bfloat16).view(b.shape)
    va.copy_(a); vb.copy_(b)
    assert vb.data_ptr() - va.data_ptr() == FAR
    return va, vb, span


@pytest.mark.parametrize('op', ['attn', 'mlp'])
def test_branch_operator_with_weights_more_than_4_gib_apart(op):
    nat, lib = native()
    E, M = 384, 256
    x = _gen(M, E, seed=31, scale=1.5) + 0.2
    gamma, beta = (1 + 0.1 * _gen(E, seed=32)).to(DEV), (0.1 * _gen(E, seed=33)).to(DEV)
    if op == 'attn':
        Wa, Wb = (_gen(3 * E, E, seed=34) * 1.5 / E ** 0.5).bfloat16().to(DEV), (_gen(E, E, seed=35) / E ** 0.5).bfloat16().to(DEV)
        ba, bb = (0.1 * _gen(3 * E, seed=36)).to(DEV), (0.1 * _gen(E, seed=37)).to(DEV)
        call, variant = lib.parseq_op_attn_fused, 1
    else:
        Wa, Wb = (_gen(4 * E, E, seed=34) / E ** 0.5).bfloat16().to(DEV), (_gen(E, 4 * E, seed=35) / (4 * E) ** 0.5).bfloat16().to(DEV)
        ba, bb = (0.1 * _gen(4 * E, seed=36)).to(DEV), (0.1 * _gen(E, seed=37)).to(DEV)
        call, variant = lib.parseq_op_mlp_variant, 11

    def run(wa, wb):
        xd = x.to(DEV).clone()
        nat.check(call(nat.ptr(xd), nat.ptr(gamma), nat.ptr(beta), nat.ptr(wa), nat.ptr(ba), nat.ptr(wb), nat.ptr(bb), M, variant, nat.stream_ptr()))
        torch.cuda.synchronize()
        return xd

    # neighbours: both matrices in one small allocation
    pack = torch.empty(Wa.numel() + Wb.numel(), dtype=torch.bfloat16, device=DEV)
    na, nb = pack[:Wa.numel()].view(Wa.shape), pack[Wa.numel():].view(Wb.shape)
    na.copy_(Wa); nb.copy_(Wb)
    want = run(na, nb)
    fa, fb, span = _far_apart(Wa, Wb)
    got = run(fa, fb)
    assert not torch.isnan(got).any() and not torch.equal(got, x.to(DEV))
    assert torch.equal(got, want)
    # the second matrix BELOW the first
    lo = torch.empty(FAR + Wa.numel() * 2, dtype=torch.uint8, device=DEV)
    wb_lo = lo[:Wb.numel() * 2].view(torch.bfloat16).view(Wb.shape)
    wa_hi = lo[FAR:FAR + Wa.numel() * 2].view(torch.bfloat16).view(Wa.shape)
    wb_lo.copy_(Wb); wa_hi.copy_(Wa)
    assert torch.equal(run(wa_hi, wb_lo), want)
    del span, lo
