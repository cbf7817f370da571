"""The CRC verdict of a tile is read behind K2 and the enqueued consumers (csrc/tiles.hip finish_crc_tile): a tile is handed to them when its last phase 2 is
done, while the CRC pass of its last chunk still runs. Whatever K2 or a consumer makes of a damaged payload in the meantime, the job must fail with the
reference's read error for that BGZF block, never with a record error and never with a result - in a single tile and in a stream of two-member tiles (21 tiles over
three buffers: phase 2 of tile t + 3 waits for the CRC pass of tile t)."""
import numpy as np
import pytest

import oracle_lib as O
import k1sched_cases as K

pytestmark = pytest.mark.gpu
ngsqc = __import__("importlib").import_module("ngs-bits_amd")

N_DATA = 41        # data members behind the header member: 42 members, so two-member tiles end with the tile {40, 41}; three records of 197 bytes each, stored blocks: a flipped byte leaves a valid stream
REC = 197          # 4 + 32 + 7 (name) + 4 (CIGAR) + 50 (SEQ) + 100 (QUAL)
QUAL0 = 97         # first quality byte of a record
# (member, payload offset): the open inflates the first eight members for the header, the damage lies behind them
DAMAGE = {
    "last_member_last_byte": (N_DATA, 3 * REC - 1),
    "last_tile": (N_DATA - 1, QUAL0 + 3),          # in the last tile, not the file's last member
    "middle_tile": (20, REC + QUAL0 + 50),
    "block_size": (21, REC),           # the second record's block_size: 193 -> 209, the chain walk leaves the records (K2 fails too)
}


def _flip(image, member_index, at):
    img = bytearray(image); pos = 0
    for _ in range(member_index):
        pos += int.from_bytes(img[pos + 16:pos + 18], "little") + 1
    img[pos + 18 + 5 + at] ^= 0x10   # 5 = stored-block header
    return bytes(img)


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    d = tmp_path_factory.mktemp("crc_late")
    img = K.records_bam([100] * (3 * N_DATA), seed=51, level=0, per_member=3)
    p = str(d / "good.bam"); open(p, "wb").write(img)
    bed = str(d / "roi.bed"); open(bed, "w").write(K.BED_TEXT)
    ob = O.Bam(p)
    assert ob.count == 3 * N_DATA
    return img, bed, O.mapping(ob, ngsqc.MODE_WGS, bed, merge_bed=False)


@pytest.mark.parametrize("tile_members", [None, "2"])
@pytest.mark.parametrize("case", sorted(DAMAGE))
def test_crc_verdict_read_behind_k2(good, monkeypatch, case, tile_members):
    img, bed, exp = good
    if tile_members:
        monkeypatch.setenv("NGSQC_TILE_MEMBERS", tile_members)
    m, at = DAMAGE[case]
    bad = _flip(img, m, at)
    assert sum(a != b for a, b in zip(bad, img)) == 1
    h = ngsqc.Handle(data=np.frombuffer(bad, dtype=np.uint8))
    with pytest.raises(ngsqc.NgsqcError) as ei:
        K.job(ngsqc, h, bed)
    assert "Could not read next alignment" in str(ei.value) and f"CRC32 mismatch in block {m}" in str(ei.value) and ei.value.code == -2, str(ei.value)
    # the handle is left reusable: the same error again, not a stale tile
    with pytest.raises(ngsqc.NgsqcError) as ei:
        K.job(ngsqc, h, bed)
    assert f"CRC32 mismatch in block {m}" in str(ei.value)
    h.close()
    g = ngsqc.Handle(data=np.frombuffer(img, dtype=np.uint8))
    out = K.job(ngsqc, g, bed)
    assert tile_members is None or g.timings()["n_tiles"] == (N_DATA + 1) // 2   # 21 tiles of two members: the last one holds members 40 and 41
    K.assert_counters(out["counters"], exp)
    g.close()


@pytest.mark.parametrize("tile_members", [None, "2"])
def test_without_the_crc_check_k2_reports_the_damaged_block_size(good, monkeypatch, tile_members):
    img, bed, _ = good
    monkeypatch.setenv("NGSQC_VERIFY_CRC", "0")
    if tile_members:
        monkeypatch.setenv("NGSQC_TILE_MEMBERS", tile_members)
    h = ngsqc.Handle(data=np.frombuffer(_flip(img, *DAMAGE["block_size"]), dtype=np.uint8))
    with pytest.raises(ngsqc.NgsqcError) as ei:
        K.job(ngsqc, h, bed)
    assert "Could not read next alignment" in str(ei.value) and "CRC32" not in str(ei.value) and ei.value.code == -2, str(ei.value)
    h.close()
