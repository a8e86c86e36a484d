import numpy as np

from conftest import golden, load_pkg


def test_spec_counts():
    s = load_pkg("synth")
    for c in (32, 48):
        spec = s.hrnet_state_spec(c, 17)
        assert len(spec) == 1754
        convs = [x for x in spec if x[2] == "conv"]
        assert len(convs) == 293
    n32 = sum(int(np.prod(sh)) for _, sh, k in s.hrnet_state_spec(32, 17) if k != "bn_count")
    n48 = sum(int(np.prod(sh)) for _, sh, k in s.hrnet_state_spec(48, 17) if k != "bn_count")
    # 28.54 M / 63.60 M parameters + BN running stats
    assert 28.4e6 < n32 < 28.8e6 and 63.4e6 < n48 < 63.9e6


def test_deterministic():
    s = load_pkg("synth")
    a, b = s.synth_state_dict(32, 17, 5), s.synth_state_dict(32, 17, 5)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["conv1.weight"], s.synth_state_dict(32, 17, 6)["conv1.weight"])


def test_spec_matches_reference_state_dict():
    """key order and shapes of the reference's own ``HRNet(c, 17).state_dict()``, stored by
    tests/golden/make_state_spec_golden.py"""
    g = golden("reference_state_specs")
    s = load_pkg("synth")
    for c in (32, 48):
        spec = s.hrnet_state_spec(c, 17)
        assert [k for k, _, _ in spec] == list(g["HRNet_%d_keys" % c])
        assert ["x".join(map(str, sh)) for _, sh, _ in spec] == list(g["HRNet_%d_shapes" % c])
