"""Host-side pieces of the wide-rank text-encoder LoRA: the padded layout's dimensions and the rank limit of the run-directory reader."""
import json

import pytest


def test_wide_layout_dimensions():
    from textboost_amd import ops
    for r in range(9, 65):
        rp, Rp = ops.lora_wide_dims(r)
        assert rp >= r and rp % 32 == 0 and rp - r < 32          # every 32-wide MFMA tile lies inside one adapter
        assert Rp >= 3 * rp and Rp % 64 == 0 and Rp - 3 * rp < 64  # the GEMMs' K granularity
    assert ops.lora_wide_dims(16) == (32, 128) and ops.lora_wide_dims(32) == (32, 128) and ops.lora_wide_dims(64) == (64, 192)
    for r in (8, 65):
        with pytest.raises(AssertionError):
            ops.lora_wide_dims(r)


@pytest.mark.parametrize("r,ok", [(64, True), (65, False), (128, False)])
def test_reader_rank_limit(tmp_path, r, ok):
    """generate.read_run_dir: rank <= 64 passes the configuration checks (and then fails on the missing weights file), above it is refused in the
    reader's words"""
    from textboost_amd import generate as G
    te_dir = tmp_path / "run" / "text_encoder"
    te_dir.mkdir(parents=True)
    json.dump({"r": r, "lora_alpha": r, "target_modules": ["q_proj", "k_proj", "v_proj"]}, open(te_dir / "adapter_config.json", "w"))
    if ok:
        with pytest.raises(FileNotFoundError):
            G.read_run_dir(str(tmp_path / "run"))
    else:
        with pytest.raises(NotImplementedError, match=f"rank-{r} adapters are not built"):
            G.read_run_dir(str(tmp_path / "run"))
