"""ops.join_exists on the reference path, and the fused-probe switch."""
import numpy as np
import pytest
import torch

from auron_amd import dtypes, ops
from auron_amd.column import Column
from auron_amd.config import JOIN_FUSED_PROBE, AuronConf


def _cols(n, key_range, seed, with_strings):
    rng = np.random.default_rng(seed)
    ints = [None if rng.random() < 0.1 else int(v)
            for v in rng.integers(0, key_range, n)]
    cols = [Column.from_pylist(ints, dtypes.int64)]
    if with_strings:
        words = ["", "a", "bb", "ccc"]
        ss = [None if rng.random() < 0.1 else words[i]
              for i in rng.integers(0, len(words), n)]
        cols.append(Column.from_pylist(ss, dtypes.string))
    return cols


@pytest.mark.parametrize("with_strings", [False, True])
@pytest.mark.parametrize("n_build,n_probe", [(0, 50), (1, 50), (300, 0), (300, 1000)])
def test_join_exists_ref_equals_counts(n_build, n_probe, with_strings):
    build = _cols(n_build, 40, 1, with_strings)
    probe = _cols(n_probe, 60, 2, with_strings)
    got = ops.join_exists(build, probe)
    assert got.dtype == torch.bool and got.shape == (n_probe,)
    assert torch.equal(got, ops.join_counts(build, probe) > 0)
    if n_build == 300 and n_probe:  # every key value is on the build side
        assert bool(got.any()) and not bool(got.all())


def test_join_exists_ref_ignores_table_argument():
    build, probe = _cols(100, 30, 3, False), _cols(200, 40, 4, False)
    assert ops.join_build(build) is None  # no native table on the CPU path
    assert torch.equal(ops.join_exists(build, probe, table=None),
                       ops.join_counts(build, probe) > 0)


def test_fused_probe_option_round_trips(monkeypatch):
    assert JOIN_FUSED_PROBE.key == "spark.auron.join.fusedProbe.enable"
    assert JOIN_FUSED_PROBE.env == "AURON_JOIN_FUSED_PROBE"
    assert AuronConf.options()[JOIN_FUSED_PROBE.key] is JOIN_FUSED_PROBE
    monkeypatch.delenv("AURON_JOIN_FUSED_PROBE", raising=False)
    assert AuronConf().get(JOIN_FUSED_PROBE) is JOIN_FUSED_PROBE.default
    for raw, want in (("0", False), ("false", False), ("1", True)):
        monkeypatch.setenv("AURON_JOIN_FUSED_PROBE", raw)
        assert AuronConf().get(JOIN_FUSED_PROBE) is want
    # a programmatic value wins over the environment
    monkeypatch.setenv("AURON_JOIN_FUSED_PROBE", "0")
    conf = AuronConf({JOIN_FUSED_PROBE.key: True})
    assert conf.get(JOIN_FUSED_PROBE) is True
    assert AuronConf().set(JOIN_FUSED_PROBE.key, False).get(JOIN_FUSED_PROBE) is False
