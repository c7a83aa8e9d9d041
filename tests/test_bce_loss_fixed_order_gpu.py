"""sam_bce_loss sums its loss in a fixed order: launch after launch the same bits, on grids of several hundred blocks with masked rows among them (an fp32
atomicAdd per block landed in arrival order, and two Trainers stepping on one batch in one process differed by an ulp in their first loss); the value
against fp64; the ticket counter is back at zero for the next launch; grids past the scratch area's 16384 parts keep the atomic sum and stay correct."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _case(r, v, no, seed):
    g = torch.Generator().manual_seed(seed)
    fixed, ocr = torch.randn(r, v, generator=g) * 3, torch.randn(r, no, generator=g) * 3
    targets = (torch.rand(r, v + no, generator=g) < 0.01).float() * torch.rand(r, v + no, generator=g)
    mask = (torch.rand(r, generator=g) < 0.5).float()
    mask[0], mask[-1] = 1.0, 0.0
    x = torch.cat([fixed, ocr], 1).double()
    bce = torch.clamp(x, min=0) - x * targets.double() + torch.log1p(torch.exp(-x.abs()))
    ref = float((bce.sum(1) * mask.double()).sum() / max(float(mask.sum()), 1.0))
    return [t.cuda() for t in (fixed, ocr, targets, mask)], ref


@pytest.mark.parametrize("r,v,no", [(768, 500, 50), (96, 5000, 50), (9, 60, 9), (5, 7, 3)])      # 768 x 1 and 96 x 8 blocks; the failing Trainer's shape; odd widths (one column per thread)
def test_loss_is_bit_identical_launch_after_launch(r, v, no):
    from sam_textvqa_amd import ops
    (fixed, ocr, targets, mask), ref = _case(r, v, no, 3)
    first = ops.bce_loss(fixed, ocr, targets, mask)
    assert abs(first[0].item() - ref) <= 1e-5 * abs(ref), (first[0].item(), ref)
    for _ in range(20):
        again = ops.bce_loss(fixed, ocr, targets, mask)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]) and torch.equal(again[2], first[2])
    masked = mask == 0
    assert (first[1][masked] == 0).all() and (first[2][masked] == 0).all()


def test_grids_past_the_scratch_area_keep_the_atomic_sum():
    from sam_textvqa_amd import ops
    (fixed, ocr, targets, mask), ref = _case(20000, 8, 2, 5)          # 20000 blocks > 16384 parts
    loss, d_fixed, d_ocr = ops.bce_loss(fixed, ocr, targets, mask)
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref), (loss.item(), ref)
    assert (d_fixed[mask == 0] == 0).all() and (d_ocr[mask == 0] == 0).all()
    (f2, o2, t2, m2), ref2 = _case(9, 60, 9, 6)                       # and a small launch right behind it sums in fixed order again
    assert abs(ops.bce_loss(f2, o2, t2, m2)[0].item() - ref2) <= 1e-5 * abs(ref2)
