"""ff_dropout / attn_dropout of the Performer (reference run_transformer.py:83-84, src/networks/transformers/performer.py:95-96,212-213), host side: the
constructor accepts 0 <= p < 1 and names the flag otherwise, and the Python restatement of the counter-based keep function of csrc/dropout.h reproduces the
published Philox4x32-10 test vectors (Random123 kat_vectors; rocRAND uses the same engine)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dropout_ref import keep_mask, philox4x32_10, threshold  # noqa: E402


def _performer(**kw):
    from synthanatomy_amd.networks.transformers.img2seq_ordering import Ordering
    from synthanatomy_amd.networks.transformers.performer import Performer
    o = Ordering("raster_scan", 3, (1, 2, 3, 4), (False,) * 3, (), ())
    return Performer(num_tokens=33, max_seq_len=24, dim=32, depth=2, heads=4, ordering=o, dim_head=64, local_attn_heads=2, local_window_size=6, **kw)


def test_dropout_flags_construct():
    net = _performer(ff_dropout=0.1, attn_dropout=0.2)
    assert net.performer.ff_dropout == pytest.approx(0.1) and net.performer.attn_dropout == pytest.approx(0.2)
    assert [l.site for l in net._chain.layers] == [0, 4]
    assert net.last_dropout_seed is None


@pytest.mark.parametrize("flag", ["ff_dropout", "attn_dropout"])
@pytest.mark.parametrize("p", [1.0, -0.1, 1.5])
def test_dropout_out_of_range_names_the_flag(flag, p):
    with pytest.raises(ValueError, match=flag):
        _performer(**{flag: p})


def test_other_unsupported_options_still_raise():
    with pytest.raises(NotImplementedError):
        _performer(ff_dropout=0.1, generalized_attention=True)


def test_philox_known_answers():
    # Random123 kat_vectors, philox4x32_10
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_keep_function_indexing_and_threshold():
    seed, site = 0x0123456789ABCDEF, 7
    words = philox4x32_10((0, 0, site, 0), (0x89ABCDEF, 0x01234567)) + philox4x32_10((1, 0, site, 0), (0x89ABCDEF, 0x01234567))
    thr = threshold(0.5)
    assert thr == 2 ** 31 and threshold(0.0) == 0
    assert keep_mask(seed, site, 0, 8, 0.5).tolist() == [w >= thr for w in words]
    # an index window starting inside a group of four reads the same words
    assert keep_mask(seed, site, 3, 4, 0.5).tolist() == [w >= thr for w in words[3:7]]
    m = keep_mask(1, 2, 0, 40000, 0.25)
    assert abs(m.mean() - 0.75) < 4 * np.sqrt(0.25 * 0.75 / m.size)
    assert not np.array_equal(m, keep_mask(1, 3, 0, 40000, 0.25)) and not np.array_equal(m, keep_mask(2, 2, 0, 40000, 0.25))
