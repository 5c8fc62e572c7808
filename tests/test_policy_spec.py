"""rsoccer_amd.vec.policy.MLPPolicy (no GPU): the parameter layout of rsx_policy_mlp is torch's own, the reference forward pass is
the equivalent module's, and bad shapes are refused."""
import itertools

import pytest

# (obs_dim, act_dim) of the registered tasks: VSS-v0, SSLStaticDefenders, SSLDribbling, SSLContestedPossession, SSLPassEndurance
# (the issue's table), and SSLContestedPossession as the 1v1 handle reports it
TASK_DIMS = [(40, 2), (24, 5), (21, 4), (24, 5), (16, 3), (14, 5)]


def _module(torch, pol):
    act = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh}[pol.hidden_act]
    layers, n_in = [], pol.obs_dim
    for _ in range(pol.layers):
        layers += [torch.nn.Linear(n_in, pol.hidden), act()]
        n_in = pol.hidden
    layers.append(torch.nn.Linear(n_in, pol.act_dim))
    if pol.out_act == "tanh":
        layers.append(torch.nn.Tanh())
    else:
        layers.append(torch.nn.Hardtanh(-1.0, 1.0))
    return torch.nn.Sequential(*layers)


@pytest.mark.parametrize("layers,hidden", list(itertools.product((1, 2), (32, 64))))
def test_num_params_for_every_shape_and_task(layers, hidden):
    from rsoccer_amd.vec.policy import MLPPolicy
    for od, ad in TASK_DIMS:
        pol = MLPPolicy(od, ad, hidden=hidden, layers=layers)
        want = hidden * od + hidden + (hidden * hidden + hidden if layers == 2 else 0) + ad * hidden + ad
        assert pol.num_params == want, (od, ad)
        assert sum(1 for _ in pol.shapes) == 2 * (layers + 1)
    assert MLPPolicy(40, 2).num_params == 64 * 40 + 64 + 64 * 64 + 64 + 2 * 64 + 2   # the defaults: 2 x 64


@pytest.mark.parametrize("layers,hidden,hact,oact", [(1, 32, "relu", "clip"), (2, 64, "tanh", "tanh"), (2, 32, "tanh", "clip"),
                                                     (1, 64, "relu", "tanh")])
def test_pack_is_parameters_to_vector_and_forward_is_the_module(layers, hidden, hact, oact):
    import torch
    from rsoccer_amd.vec.policy import MLPPolicy
    torch.manual_seed(3)
    pol = MLPPolicy(21, 4, hidden=hidden, layers=layers, hidden_act=hact, out_act=oact)
    mod = _module(torch, pol).double()
    lin = [m for m in mod if isinstance(m, torch.nn.Linear)]
    vec = torch.nn.utils.parameters_to_vector(mod.parameters()).detach()
    packed = pol.pack([t for m in lin for t in (m.weight, m.bias)])
    assert packed.dtype == torch.float32 and torch.equal(packed, vec.float())
    assert torch.equal(pol.from_module(mod), packed)
    parts = pol.unpack(vec)
    assert [tuple(p.shape) for p in parts] == pol.shapes
    for p, q in zip(parts, [t for m in lin for t in (m.weight, m.bias)]):
        assert torch.equal(p, q.detach())
    assert [tuple(p.shape) for p in pol.unpack(torch.zeros(7, pol.num_params))] == [(7,) + s for s in pol.shapes]
    obs = torch.rand(5, 3, 21, dtype=torch.float64) * 2.4 - 1.2
    got = pol.forward(obs, vec)
    assert got.dtype == torch.float64 and got.shape == (5, 3, 4)
    assert torch.allclose(got, mod(obs).detach(), rtol=0, atol=1e-14)
    assert pol.forward(obs, vec, dtype=torch.float32).dtype == torch.float32
    assert float(got.abs().max()) <= 1.0


def test_bad_specs_raise():
    import torch
    from rsoccer_amd.vec.policy import MLPPolicy
    for kw in (dict(hidden=48), dict(hidden=128), dict(layers=0), dict(layers=3), dict(hidden_act="gelu"), dict(hidden_act="clip"),
               dict(out_act="relu"), dict(out_act="none")):
        with pytest.raises(ValueError):
            MLPPolicy(40, 2, **kw)
    for od, ad in ((0, 2), (40, 0)):
        with pytest.raises(ValueError):
            MLPPolicy(od, ad)
    pol = MLPPolicy(40, 2)
    with pytest.raises(ValueError):
        pol.unpack(torch.zeros(pol.num_params - 1))
    with pytest.raises(ValueError):
        pol.pack([torch.zeros(s) for s in pol.shapes][:-1])
    with pytest.raises(ValueError):
        pol.pack([torch.zeros(s) for s in pol.shapes[:-1]] + [torch.zeros(3)])
    with pytest.raises(ValueError):
        pol.from_module(torch.nn.Sequential(torch.nn.Linear(40, 64), torch.nn.Tanh(), torch.nn.Linear(64, 2)))   # one hidden layer


def test_spec_is_the_c_struct():
    from rsoccer_amd import _lib
    from rsoccer_amd.vec.policy import MLPPolicy
    s = MLPPolicy(40, 2, hidden=32, layers=1, hidden_act="relu", out_act="clip").spec()
    assert (s.n_hidden_layers, s.hidden, s.hidden_act, s.out_act) == (1, 32, _lib.ACT_RELU, _lib.ACT_CLIP)
    s = MLPPolicy(40, 2).spec()
    assert (s.n_hidden_layers, s.hidden, s.hidden_act, s.out_act) == (2, 64, _lib.ACT_TANH, _lib.ACT_TANH)
