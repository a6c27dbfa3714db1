"""CPU tier: the two cases of plan.forward_schedule that the rendered launch plans cannot show -- a given dropout mask, and the
memo when a table look-up is swapped (the GPU tests force kernel forms that way)."""
import pytest

FLAGS = dict(use_winograd=True, fuse_expand=True, fuse_expand_wino=True, fuse_fire_bridge=True, fuse_pool_squeeze=False,
             fuse_stem_squeeze=True, fuse_train_forward=True, fused_dropout=True)


@pytest.mark.parametrize('save', [False, True])
def test_given_mask_runs_the_last_fire_as_a_plain_pair_with_ymul(save):
    from squeezedet_pytorch_amd import plan
    flags = plan.Flags(**FLAGS)
    masked = plan.forward_schedule('squeezedet', 20, (384, 1248), flags, save, 'mask')
    stream = plan.forward_schedule('squeezedet', 20, (384, 1248), flags, save, 'stream')
    none = plan.forward_schedule('squeezedet', 20, (384, 1248), flags, save, None)
    last = masked[-2]
    assert (last.expand, last.ymul, last.mask_launch) == ('plain', True, False) and not masked[-1].fused_rng
    assert (stream[-2].expand, stream[-2].ymul, stream[-2].mask_launch) == ('conv_drop', False, False) and stream[-1].fused_rng
    assert masked[:-2] == stream[:-2] == none[:-2]                 # dropout touches the last Fire only
    assert not any(st.ymul or st.mask_launch for st in none if type(st) is plan.FireStep)
    # the stream without its fused form: the stand-alone mask launch, then the same plain pair
    drawn = plan.forward_schedule('squeezedet', 20, (384, 1248), flags._replace(fused_dropout=False), save, 'stream')
    assert drawn[-2] == last._replace(mask_launch=True)


def test_memo_is_not_answered_across_a_swapped_chooser(monkeypatch):
    from squeezedet_pytorch_amd import ops, plan
    flags = plan.Flags(**FLAGS)
    before = plan.forward_schedule('squeezedet', 20, (384, 1248), flags)
    assert plan.forward_schedule('squeezedet', 20, (384, 1248), flags) is before
    assert any(st.expand == 'fire_bridge' for st in before if type(st) is plan.FireStep)
    monkeypatch.setattr(ops, 'choose_fire_bridge_cfg', lambda *a: None)
    swapped = plan.forward_schedule('squeezedet', 20, (384, 1248), flags)
    assert not any(st.expand == 'fire_bridge' for st in swapped if type(st) is plan.FireStep)
    monkeypatch.undo()
    assert plan.forward_schedule('squeezedet', 20, (384, 1248), flags) is before
