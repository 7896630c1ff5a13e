"""tests/footprint.py can fail: an image built from the oracle passes compare(), and one altered byte in a guard, in the reference
data or at the end of a completely decoded unit's output does not; a change inside masked slack does.  And the two conditions on
masking hold on a mixed list of valid and failing items.  No GPU: the image is the expected one with noise where the mask allows it."""
import numpy as np
import pytest

import crafted_streams as CS
import footprint as F
import libmspack_amd as M
import test_gpu_footprint as G

FILL = 0xA5


def three_items():
    d = G.text("mix", 129)
    comp, fo = M.lzx_encode(d, 15, 0, M.lzx_opts(mode=1))
    ref = CS._rnd(1, 17)
    s, plain = G.delta_stream(17, 1000, ref)
    z = M.gen_plaintext(90, M.TEXT_MIX, 17).tobytes()
    zs, offs = G.folder_blocks(z)
    return [F.Item("lzx", M.KIND_LZX, comp.tobytes(), 129, wb=15, tab=[0], plain=d.tobytes(), ri=3, ro=17),
            F.Item("delta", M.KIND_LZX_DELTA, s, 1000, wb=17, ref=ref, plain=plain, ri=8, ro=127),
            F.Item("mszip", M.KIND_MSZIP, zs, 17, tab=offs, plain=z, ri=13, ro=65)]


def oracle_image(items, seed=7):
    """the layout, the expected image, its mask -- and an image a correct decoder could have left: the expected bytes, noise where
    the mask says unspecified"""
    L = F.layout(items)
    wants = [F.oracle(it) for it in items]
    exp, mask = F.expected_image(L, wants, FILL)
    image = exp.copy()
    image[mask] = np.random.default_rng(seed).integers(0, 256, int(mask.sum()), dtype=np.uint8)
    return L, wants, exp, mask, image


def test_layout_is_what_the_issue_asks(built):
    items = three_items()
    L = F.layout(items)
    for it, u, (lo, ref0, out, end, hi) in zip(items, L.units, L.span):
        assert out == u["out_off"] and out % 128 == it.ro and (u["in_off"] - it.skip) % 16 == it.ri
        assert out - ref0 == len(it.ref) and ref0 - lo >= F.GUARD and hi - end == F.GUARD
        assert (L.cls[lo:ref0] == F.NOBODY).all() and (L.cls[end:hi] == F.NOBODY).all() and (L.cls[out:out + it.out_len] == F.OUTPUT).all()
        s = np.frombuffer(it.stream, dtype=np.uint8)
        a = int(u["in_off"])
        assert np.array_equal(L.arena[a:a + s.size], s) and (L.arena[a - 16:a] == 0xFF).all()
        assert (L.arena[a + s.size:a + s.size + 8] == 0xFF).all()
    assert L.span[-1][4] == L.out_bytes and (L.arena[-64:] == 0xFF).all()
    assert L.units["in_chunk"][0] * 4 % 4 == 0 and L.units["flags"][0] & M.UF_FRAME_TABLE
    assert (L.cls[L.span[2][2] + 17:L.span[2][2] + 17 + F.ZIP_SLACK] == F.SLACK).all()


def test_compare_passes_on_the_oracles_image_and_fails_on_one_byte(built):
    items = three_items()
    L, wants, exp, mask, image = oracle_image(items)
    assert all(w.err == 0 and w.out_len == it.out_len and w.data == it.plain for it, w in zip(items, wants))
    F.compare(image, exp, mask, L)
    lo, ref0, out, end, hi = L.span[1]                         # (the DELTA unit)
    spots = {"guard below": (lo + F.GUARD - 1, "a guard byte"), "guard behind": (end, "a guard byte"),
             "first guard byte": (0, "a guard byte"), "last guard byte": (L.out_bytes - 1, "a guard byte"),
             "reference": (ref0, "reference data"), "last reference byte": (out - 1, "reference data"),
             "last owned byte": (out + items[1].out_len - 1, "output"),
             "last output byte of the MSZIP unit": (L.span[2][2] + 16, "output")}
    for what, (p, cls) in spots.items():
        broken = image.copy()
        broken[p] ^= 0x01
        with pytest.raises(AssertionError) as e:
            F.compare(broken, exp, mask, L)
        msg = str(e.value)
        assert "byte %d of" % p in msg and cls in msg and "1 bytes differ" in msg, (what, msg)
        assert ("(%s)" % L.items[int(L.owner[p])].name) in msg and "out_off % 128 = " in msg, (what, msg)
    # masked: the MSZIP unit's slack
    z_out = L.span[2][2]
    assert mask[z_out + 17:z_out + 17 + F.ZIP_SLACK].all()
    ok = image.copy()
    ok[z_out + 17] ^= 0xFF; ok[z_out + 17 + F.ZIP_SLACK - 1] ^= 0xFF
    F.compare(ok, exp, mask, L)
    broken = image.copy()
    broken[z_out + 17 + F.ZIP_SLACK] ^= 0x80                   # ... and the first byte behind it is nobody's
    with pytest.raises(AssertionError, match="a guard byte"):
        F.compare(broken, exp, mask, L)


def test_masking_conditions_on_valid_and_failing_items(built):
    """nothing of a completely decoded unit's output is masked and nothing outside owned regions ever is (expected_image asserts
    both; here they are looked at from outside, on truncated and hand-built failing units, marks, logs and KWAJ framing)"""
    items = three_items() + G.truncation_items("lzx")[::7] + G.truncation_items("qtm")[::5] + G.mszip_items()[-4:] + \
        G.qtm_items()[28:30] + G.log_items()[:2] + [it for it in G.crafted_items("lzx")[1] if it.plain is None][:6] + \
        [it for it in G.crafted_items("mszip")[1] if it.plain is None][:4]
    L, wants, exp, mask, image = oracle_image(items)
    assert sum(1 for w in wants if w.err) >= 8 and sum(1 for w in wants if not w.err) >= 8
    owned = np.zeros(L.out_bytes, dtype=bool)
    for it, (lo, ref0, out, end, hi), w in zip(items, L.span, wants):
        for a, b, _c in it.owned(out):
            owned[a:b] = True
        if w.err == 0 and w.out_len == it.out_len:
            assert not mask[out:out + it.out_len].any(), it.name
        assert not mask[lo:out].any() and not mask[end:hi].any(), it.name
        if w.trusted:
            assert not mask[out:out + min(w.out_len, it.out_len)].any(), it.name
    assert not (mask & ~owned).any()
    assert (exp[~owned & (L.cls != F.REFERENCE)] == FILL).all()
    F.compare(image, exp, mask, L)
