"""CPU model of the LDS image of the DMA-staged persistent packed GEMM (gemm_hlp_kernel<.., DMA>,
csrc/gemm_hl.hip): who fetches which 16-byte chunk of a 256 x 32 slab, where it lands in LDS, and
which bytes a fragment lane reads.  The kernel's index expressions are copied from here.

A slab of one operand is 256 plane rows x one 128-byte line (8 chunks of 16 bytes: chunk c is plane
(c >> 1) & 1, reduction chunk 2 (c >> 2) + (c & 1)).  An LDS-DMA wave instruction writes
64 x 16 bytes CONTIGUOUSLY at a wave-uniform base, so the image is cut into 1 KB pieces of
8 rows x 8 chunks and the swizzle sits on the SOURCE side: position p (= lane) of piece P holds
row 8 P + (p >> 3), chunk (p & 7) ^ s(row), s(row) = (row >> 1) & 7 -- i.e. the image is
[256 rows][128 bytes] with the chunk index XORed by (row >> 1) & 7.  Eight consecutive lanes still
fetch one whole 128-byte line, as the register-staged loader does.

Chunk-major pieces with a one-bit XOR of the piece index (position p = row p & 7, chunk
(p >> 3) ^ (P & 1)) spread 16 CONSECUTIVE lanes over the 16 bank groups, but ds_read_b128 is
serviced in the lane groups {0-3, 12-15, 20-27}, ... (below): there lanes 12-15 and 20-23 meet in
the same four bank groups.  test_chunk_major_layout_conflicts_in_the_hardware_groups keeps that on
record; the layout above is free of conflicts under both groupings.
"""
import itertools

ROWS, CHUNKS, PIECE = 256, 8, 1024
WAVES, WN, MI, NJ = 8, 4, 4, 2

# ds_read_b128: four lane groups of 16, one LDS cycle each when no two lanes of a group share one of
# the 16 bank groups of 16 bytes (256-byte bank row)
HW_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
             list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
             list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
             list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
SEQ_GROUPS = [list(range(16 * g, 16 * g + 16)) for g in range(4)]


def hl256_slot(row, kc):
    """The register-staged image: half index of reduction chunk kc of `row` within ONE plane."""
    return row * 32 + ((kc ^ ((0x78 >> (2 * ((row >> 2) & 3))) & 3)) << 3)


def line_chunk(plane, kc):
    """Chunk of the 128-byte slab line that holds reduction chunk kc (8 indices) of a plane."""
    return 4 * (kc >> 1) + 2 * plane + (kc & 1)


# ---- the kernel's expressions

def swz(row):
    return (row >> 1) & 7


def a_pieces(wave):
    """A is private to a row of waves (rows 128 wm ..): region (wm, h) = the 64 rows its waves read
    in half-step h; a wave stages two pieces of each.  P & 1 == wn & 1 for every piece of a wave."""
    wm, wn = wave // WN, wave % WN
    return [[wm * 16 + 8 * h + 4 * q + wn for q in range(2)] for h in range(2)]


def b_pieces(wave):
    return [8 * i + wave for i in range(4)]


def lane_source(wave, piece, lane):
    """(row, chunk of the line) lane `lane` of `wave` fetches for `piece`: one per-lane offset for
    all pieces of a wave, the piece's rows are a scalar offset."""
    wn = wave % WN
    l8 = lane >> 3
    cs = (lane & 7) ^ ((l8 >> 1) | ((wn & 1) << 2))
    return 8 * piece + l8, cs


def lane_dest(piece, lane):
    return PIECE * piece + 16 * lane            # M0 = the piece, + 16 bytes per lane


def frag_addr(row16, frow, fk, plane):
    """Byte a fragment lane (frow = lane & 15, fk = lane >> 4) reads: row row16 + frow."""
    ch = 4 * (fk >> 1) + (fk & 1)
    fro = 128 * frow + 16 * ((ch ^ (frow >> 1)) & 7)
    return 128 * row16 + (fro ^ (32 * plane))


def a_frag_rows(wave):
    wm = wave // WN
    return [[wm * 32 * MI + (hf * MI + i) * 16 for i in range(MI)] for hf in range(2)]


def b_frag_rows(wave):
    wn = wave % WN
    return [wn * 32 * NJ + j * 16 for j in range(2 * NJ)]


def build_image(pieces_of):
    """byte address of a 16-byte granule -> (row, line chunk) written there, over all waves."""
    image = {}
    for wave in range(WAVES):
        for piece in pieces_of(wave):
            for lane in range(64):
                dst = lane_dest(piece, lane)
                assert dst not in image
                image[dst] = lane_source(wave, piece, lane)
    return image


def a_pieces_flat(wave):
    return list(itertools.chain.from_iterable(a_pieces(wave)))


IMAGES = {'A': build_image(a_pieces_flat), 'B': build_image(b_pieces)}


def test_every_chunk_of_a_slab_is_written_exactly_once():
    for name, image in IMAGES.items():
        assert len(image) == ROWS * CHUNKS, name
        assert sorted(image) == [16 * g for g in range(ROWS * CHUNKS)], name       # dense, 32 KB
        assert sorted(image.values()) == [(r, c) for r in range(ROWS) for c in range(CHUNKS)], name


def test_one_lane_offset_serves_every_piece_of_a_wave():
    """(row within the piece, chunk) is the same for all pieces a wave stages: the kernel keeps one
    offset register per operand and moves from piece to piece with the scalar offset."""
    for wave in range(WAVES):
        for pieces in (a_pieces_flat(wave), b_pieces(wave)):
            per_lane = {tuple((lane_source(wave, p, lane)[0] - 8 * p, lane_source(wave, p, lane)[1])
                              for lane in range(64)) for p in pieces}
            assert len(per_lane) == 1


def test_the_lane_expression_is_the_row_swizzle():
    """The kernel never forms the row: (lane >> 4) | (wn & 1) << 2 is swz(row) for its pieces."""
    for wave in range(WAVES):
        for p in a_pieces_flat(wave) + b_pieces(wave):
            for lane in range(64):
                row, cs = lane_source(wave, p, lane)
                assert cs == (lane & 7) ^ swz(row)


def test_a_wave_instruction_fetches_eight_whole_lines():
    for wave in range(WAVES):
        for p in a_pieces_flat(wave) + b_pieces(wave):
            for l8 in range(8):
                got = [lane_source(wave, p, 8 * l8 + e) for e in range(8)]
                assert {r for r, _ in got} == {8 * p + l8}
                assert sorted(c for _, c in got) == list(range(8))


def test_a_regions_are_private_to_their_wave_row_and_half_step():
    """The ordering rules of the K loop lean on this: the A rows a wave stages for half-step h are
    read by waves of its own row in half-step h only."""
    for wave in range(WAVES):
        wm = wave // WN
        for h in range(2):
            for p in a_pieces(wave)[h]:
                assert wm * 128 + 64 * h <= 8 * p < wm * 128 + 64 * h + 64
    for wave in range(WAVES):
        wm = wave // WN
        for hf in range(2):
            for row16 in a_frag_rows(wave)[hf]:
                assert wm * 128 + 64 * hf <= row16 < wm * 128 + 64 * hf + 64


def test_fragment_lanes_read_what_the_register_staged_image_gives_them():
    """hl256_slot(row, fk) of plane `plane` holds reduction chunk fk of that plane; the new read of
    the same lane must find the line chunk that carries exactly that."""
    for name, rows_of in (('A', lambda w: list(itertools.chain.from_iterable(a_frag_rows(w)))),
                          ('B', b_frag_rows)):
        image = IMAGES[name]
        for wave in range(WAVES):
            for row16 in rows_of(wave):
                for lane in range(64):
                    frow, fk = lane & 15, lane >> 4
                    for plane in range(2):
                        # today: the chunk stored at hl256_slot is the one the loader put there
                        c_line = line_chunk(plane, fk)
                        assert (c_line >> 1) & 1 == plane
                        assert 2 * (c_line >> 2) + (c_line & 1) == fk
                        slot = hl256_slot(row16 + frow, fk)
                        assert slot // 32 == row16 + frow                   # same row today
                        addr = frag_addr(row16, frow, fk, plane)
                        assert addr % 16 == 0 and 0 <= addr < ROWS * 128
                        assert image[addr] == (row16 + frow, c_line), (name, wave, row16, lane)


def _conflicts(addr_of_lane, groups):
    bad = 0
    for grp in groups:
        banks = [(addr_of_lane(lane) // 16) % 16 for lane in grp]
        bad += len(banks) - len(set(banks))
    return bad


def test_no_ds_read_b128_lane_group_shares_a_bank_group():
    for groups in (HW_GROUPS, SEQ_GROUPS):
        for row16 in range(0, ROWS, 16):
            for plane in range(2):
                assert _conflicts(lambda l: frag_addr(row16, l & 15, l >> 4, plane), groups) == 0


def test_chunk_major_layout_conflicts_in_the_hardware_groups():
    """The layout first proposed for this kernel: piece position p = row p & 7, chunk
    (p >> 3) ^ (P & 1).  Free of conflicts for 16 consecutive lanes, two-way in the groups the LDS
    services -- why it was not used."""
    def addr(row16, lane, plane):
        r = row16 + (lane & 15)
        c = line_chunk(plane, lane >> 4)
        return 1024 * (r >> 3) + 16 * (8 * (c ^ ((r >> 3) & 1)) + (r & 7))
    assert _conflicts(lambda l: addr(0, l, 0), SEQ_GROUPS) == 0
    assert _conflicts(lambda l: addr(0, l, 0), HW_GROUPS) > 0
