"""CPU: the device-masks option is off by default, needs the device path, and shows in the CLI's plan only when asked for; nothing
here touches a GPU (the route itself is tests/test_device_masks_gpu.py's)."""
import json

import pytest

from unopose_amd import cli
from unopose_amd import provider as P

BASE = dict(model=dict(cfg={}), dataloader=dict(test=dict(dataset=dict(cfg={}, eval_dataset_name="ycbv", detetion_path="dets.json"))),
            test=dict(amp=dict(enabled=False), instance_batch_size=16), misc=dict(output_dir="output/unopose", load_from="/x/ckpt_12.pth"), bop_eval=dict(split="test"))


def test_device_masks_needs_the_device_path(tmp_path, capsys):
    with pytest.raises(ValueError, match="device_masks needs"):
        P.BOPTestsetOneRef({}, "ycbv", "none.json", device_masks=True)
    cfgf = tmp_path / "cfg.json"
    cfgf.write_text(json.dumps(BASE))
    with pytest.raises(SystemExit):
        cli.main(["--config-file", str(cfgf), "--device-masks", "--print-plan"])
    assert "--device-masks requires --device-prep" in capsys.readouterr().err
    plans = []
    for flags in (["--device-prep"], ["--device-prep", "--device-masks"]):
        assert cli.main(["--config-file", str(cfgf), "--print-plan", *flags]) == 0
        plans.append(json.loads(capsys.readouterr().out.strip().splitlines()[-1]))
    assert "device_masks" not in plans[0] and plans[1] == dict(plans[0], device_masks=True)
