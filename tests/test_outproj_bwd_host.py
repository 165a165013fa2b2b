"""Host side of rs_outproj_bwd_bf16 (no GPU): workspace sizing on wgrad_bf16's row split, argument
checks, and its work model for bench.py --full."""
import pytest

from recommendsystemproject_amd import _hip, profiling


def test_ws_bytes_follow_the_weight_gradient_split():
    L = _hip.lib()
    # C2's token layer: 416-row workgroups -> 493 partial rows [dW 64 x 64 | db 64]
    assert L.rs_outproj_bwd_bf16_ws_bytes(204800, 64) == 493 * (64 * 64 + 64) * 4
    assert L.rs_outproj_bwd_bf16_ws_bytes(48, 64) == (64 * 64 + 64) * 4
    assert L.rs_outproj_bwd_bf16_ws_bytes(150, 64) == 2 * (64 * 64 + 64) * 4
    assert L.rs_outproj_bwd_bf16_ws_bytes(204800, 32) == 0  # not covered


@pytest.mark.parametrize('rows', [1, 63, 64, 4096, 32768, 35008, 204800, 1000000])
def test_ws_bytes_of_every_weight_gradient_follow_one_row_split(rows):
    """The row split every weight-gradient kernel shares: up to 512 workgroups (the cap) of at
    least 64 rows (the floor), each a whole number of 32-row chunks. The one-pass backwards size
    their workspace for the workgroups that split launches (one partial row [dW | db] each);
    rs_wgrad_ws_bytes, which serves the fp32 kernel (16-row chunks) and the bf16 one alike, for
    the workgroup count before the rounding to whole chunks, which bounds both."""
    L = _hip.lib()
    nb = min(max(rows // 64, 1), 512)
    per_wg = -(-rows // nb)               # rows of a workgroup ...
    per_wg = -(-per_wg // 32) * 32        # ... in whole 32-row chunks
    blocks = -(-rows // per_wg)
    assert blocks <= nb
    assert L.rs_outproj_bwd_bf16_ws_bytes(rows, 64) == blocks * (64 * 64 + 64) * 4
    for dcat in (24, 40, 72):
        assert L.rs_seq_input_bwd_bf16_ws_bytes(rows, 64, dcat) == blocks * (64 * dcat + 64) * 4
    assert L.rs_linear_bwd_bf16_ws_bytes(rows, 192, 64) == blocks * (192 * 64 + 192) * 4
    for Mo, No in ((64, 64), (64, 40), (192, 64), (256, 172)):
        assert L.rs_wgrad_ws_bytes(Mo, No, rows) == nb * (Mo * No + Mo) * 4


def test_bad_arguments_are_errors():
    with pytest.raises(_hip.HipError, match='d == 64'):
        _hip.call('rs_outproj_bwd_bf16', None, None, None, 64, 128, 32, 0.0, None, 0, None, None, None, None, None)
    with pytest.raises(_hip.HipError, match='null operand'):
        _hip.call('rs_outproj_bwd_bf16', None, None, None, 64, 128, 64, 0.0, None, 0, None, None, None, None, None)
    # no rows: nothing to do, nothing touched
    _hip.call('rs_outproj_bwd_bf16', None, None, None, 64, 0, 64, 0.0, None, 0, None, None, None, None, None)


def test_work_model():
    M, d = 204800, 64
    args = (1, 2, 3, 64, M, d, 0.15, 4, 17, 5, 6, 7, 8, 9)
    flop, byts = profiling.WORK['rs_outproj_bwd_bf16'](args)
    assert flop == 2 * 2.0 * M * d * d  # dW = y^T att and datt = y W
    assert byts == 3 * 4.0 * M * d      # dh and att read, datt written
