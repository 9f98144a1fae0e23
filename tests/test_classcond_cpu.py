"""CPU: class-conditional U-Nets (UNetModel(num_classes=K), ClassCondUNetModelWrapper(class_cond=True, num_classes=K)) - parameter inventory,
construction and the `y` argument rules, plus the fp32 restatement of the label path the GPU tests hold the HIP engine to.

The reference registers label_emb = nn.Embedding(num_classes, 4 * model_channels) (AD/image_diffusion/unet.py:571-572) but its
forward(x, timesteps) never reads it (unet.py:708-728), so tests/golden/unet_*_classcond.npz (tools/make_goldens_classcond.py) pin the key
order and the y=None output only.  The label term follows the upstream guided-diffusion / torchcfm rule,
emb = time_embed(timestep_embedding(t)) + label_emb(y); torchcfm is not vendored, so `classcond_forward` below restates it from the
oracle's pieces ('parity unpinned' for the label term).
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mi355.synth import synth_state_dict
from oracle import unet_ref
from tests.test_oracle_golden import cfg_from_json

CLASSCOND = ["tiny", "tiny_film_updown_neworder", "mnist"]


@dataclass
class ClassCondConfig(unet_ref.UNetConfig):
    num_classes: Optional[int] = None


def classcond_cfg(c: dict) -> ClassCondConfig:
    base = cfg_from_json(c)
    return ClassCondConfig(**{k: getattr(base, k) for k in base.__dataclass_fields__}, num_classes=c.get("num_classes"))


def classcond_forward(sd, cfg, x: torch.Tensor, t: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """UNetModel.forward with the label term: emb = time_embed(timestep_embedding(t)) + label_emb[y], then the oracle's layers (fp32,
    transparent to autograd).  y=None is the reference's forward."""
    input_blocks, middle, output_blocks, _ = unet_ref.build_plan(cfg)
    emb = F.linear(unet_ref.timestep_embedding(t, cfg.model_channels), sd["time_embed.0.weight"], sd["time_embed.0.bias"])
    emb = F.linear(F.silu(emb), sd["time_embed.2.weight"], sd["time_embed.2.bias"])
    if y is not None:
        emb = emb + sd["label_emb.weight"][y.long()]
    hs = []
    h = x.float()
    for i, layers in enumerate(input_blocks):
        h = unet_ref._run_layers(sd, cfg, f"input_blocks.{i}", layers, h, emb)
        hs.append(h)
    h = unet_ref._run_layers(sd, cfg, "middle_block", middle, h, emb)
    for i, layers in enumerate(output_blocks):
        h = torch.cat([h, hs.pop()], dim=1)
        h = unet_ref._run_layers(sd, cfg, f"output_blocks.{i}", layers, h, emb)
    h = F.silu(unet_ref.group_norm32(h, sd["out.0.weight"], sd["out.0.bias"]))
    return unet_ref._conv(sd, "out.2", h)


def load_case(golden, name):
    g = golden(f"unet_{name}_classcond")
    c = dict(g.json("config"))
    cfg = classcond_cfg(c)
    return g, cfg


@pytest.mark.parametrize("name", CLASSCOND)
def test_param_shapes_match_reference_keys(golden, name):
    """label_emb.weight [K, 4 mc] right after time_embed.2.bias, in the Python builder and in the C plan builder."""
    import ctypes as C

    from image_diffusion.unet import param_shapes
    from mi355 import _lib
    from mi355.engine import param_inventory

    g, cfg = load_case(golden, name)
    want = [(k, tuple(s)) for k, s in g.json("keys")]
    assert list(param_shapes(cfg).items()) == want
    assert want[4] == ("label_emb.weight", (cfg.num_classes, 4 * cfg.model_channels))
    assert sum(int(np.prod(s)) for _, s in want) == int(g["n_params"])
    for dt in (_lib.MI355_F32, _lib.MI355_BF16):
        c = _lib.make_config(image_size=cfg.image_size, in_channels=cfg.in_channels, model_channels=cfg.model_channels,
                             out_channels=cfg.out_channels, num_res_blocks=cfg.num_res_blocks, attention_ds=cfg.attention_resolutions,
                             channel_mult=cfg.channel_mult, conv_resample=cfg.conv_resample, num_heads=cfg.num_heads,
                             num_head_channels=cfg.num_head_channels, use_scale_shift_norm=cfg.use_scale_shift_norm,
                             resblock_updown=cfg.resblock_updown, use_new_attention_order=cfg.use_new_attention_order, dtype=dt,
                             num_classes=cfg.num_classes)
        assert param_inventory(c) == want
        assert _lib.lib().mi355_unet_param_count(C.byref(c)) == len(want)
        c.num_classes = 0   # the unconditional inventory is the same list without label_emb
        assert param_inventory(c) == [kv for kv in want if kv[0] != "label_emb.weight"]


def test_negative_num_classes_is_refused():
    import ctypes as C

    from mi355 import _lib

    with pytest.raises(ValueError):
        _lib.make_config(image_size=16, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_ds=(2,),
                         channel_mult=(1, 2), num_classes=-1)
    c = _lib.make_config(image_size=16, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_ds=(2,),
                         channel_mult=(1, 2))
    c.num_classes = -3
    assert _lib.lib().mi355_unet_param_count(C.byref(c)) < 0
    assert b"num_classes" in _lib.lib().mi355_last_error()


@pytest.mark.parametrize("name", CLASSCOND)
def test_restatement_without_labels_is_the_reference(golden, name):
    """The restated forward with y=None reproduces the reference's output on the same synthesised weights (CPU, fp32)."""
    from image_diffusion.unet import param_shapes

    g, cfg = load_case(golden, name)
    sd = synth_state_dict(param_shapes(cfg), int(g["seed"]))
    torch.testing.assert_close(classcond_forward(sd, cfg, g.t("x"), g.t("t")), g.t("y"), rtol=1e-5, atol=1e-6)
    # and the label term changes it (the fixture alone cannot tell a model that drops y)
    y = torch.arange(g.t("x").shape[0]) % cfg.num_classes
    assert (classcond_forward(sd, cfg, g.t("x"), g.t("t"), y) - g.t("y")).abs().max() > 1e-3


def test_models_construct_with_num_classes():
    from image_diffusion.unet import UNetModel
    from torchcfm_compat import ClassCondUNetModelWrapper, UNetModelWrapper

    torch.manual_seed(0)
    m = UNetModel(image_size=28, in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=(1,),
                  channel_mult=(1, 2, 2), num_classes=10)
    keys = list(m.state_dict())
    assert keys[4] == "label_emb.weight" and tuple(m.state_dict()["label_emb.weight"].shape) == (10, 128)
    w = m.state_dict()["label_emb.weight"]
    assert abs(float(w.std()) - 1.0) < 0.1 and abs(float(w.mean())) < 0.1   # nn.Embedding's N(0, 1)
    # conditional_mnist.ipynb's model (torchcfm.models.unet.UNetModel)
    wr = ClassCondUNetModelWrapper(dim=(1, 28, 28), num_channels=32, num_res_blocks=1, num_classes=10, class_cond=True)
    assert isinstance(wr, UNetModelWrapper) and wr.num_classes == 10 and "label_emb.weight" in wr.state_dict()
    assert wr._cfg_kwargs()["num_classes"] == 10
    # torchcfm gating: no class_cond -> no label embedding; the mnist/ call sites' class_cond=True, num_classes=None -> none either
    for cls in (UNetModelWrapper, ClassCondUNetModelWrapper):
        for kw in (dict(num_classes=10, class_cond=False), dict(num_classes=None, class_cond=True)):
            u = cls(dim=(1, 28, 28), num_channels=32, num_res_blocks=1, **kw)
            assert u.num_classes is None and "label_emb.weight" not in u.state_dict()
    # the cifar10/ and mnist/ stand-in keeps refusing a label embedding, and names the class that builds one
    with pytest.raises(NotImplementedError, match="ClassCondUNetModelWrapper"):
        UNetModelWrapper(dim=(1, 28, 28), num_channels=32, num_res_blocks=1, num_classes=10, class_cond=True)
    with pytest.raises(ValueError):
        UNetModel(image_size=16, in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=(2,),
                  channel_mult=(1, 2), num_classes=0)


def test_y_rules():
    """UNetModel: y on a model without num_classes is a ValueError.  Wrapper: with num_classes, y is required (ValueError naming y); without,
    y is ignored.  NeuralODE.trajectory of a class-conditional wrapper surfaces the model's y error."""
    from image_diffusion.unet import UNetModel
    from mi355._lib import MI355BackendError
    from torchcfm_compat import ClassCondUNetModelWrapper, NeuralODE, UNetModelWrapper

    x = torch.zeros(2, 1, 28, 28)
    y = torch.tensor([1, 2])
    plain = UNetModel(image_size=28, in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=(1,),
                      channel_mult=(1, 2, 2))
    with pytest.raises(ValueError, match="num_classes"):
        plain(x, torch.zeros(2), y)
    with pytest.raises(MI355BackendError):    # y=None reaches the backend check (CPU tensors: no CPU path)
        plain(x, torch.zeros(2))
    cond = ClassCondUNetModelWrapper(dim=(1, 28, 28), num_channels=32, num_res_blocks=1, num_classes=10, class_cond=True)
    with pytest.raises(ValueError, match=r"\by\b"):
        cond(0.5, x)
    with pytest.raises(MI355BackendError):
        cond(0.5, x, y)
    with pytest.raises(ValueError, match=r"\by\b"):
        NeuralODE(cond, solver="euler").trajectory(x, torch.linspace(0, 1, 3))
    uncond = UNetModelWrapper(dim=(1, 28, 28), num_channels=32, num_res_blocks=1, num_classes=None, class_cond=True)
    with pytest.raises(MI355BackendError):    # y ignored: the call gets as far as the backend check
        uncond(0.5, x, y)

