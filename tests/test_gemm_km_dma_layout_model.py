"""CPU model of the LDS image of the DMA-staged K-major packed GEMM (gemm_hlt_dma_kernel,
csrc/gemm_hl.hip): who fetches which 16-byte chunk of a 32 x 256 slab, where it lands in LDS, and
which bytes a lane of the transposing fragment read supplies.  The kernel's index expressions are
copied from here.

A slab of one K-major operand is 32 plane rows (reduction indices) x 1 KB: 16 column groups of
(16 hi, 16 lo) halfs = 64 chunks of 16 bytes; chunk c is column group c >> 2, plane (c >> 1) & 1,
columns 8 (c & 1) .. + 7 of the group.  An LDS-DMA wave instruction writes 64 x 16 bytes
CONTIGUOUSLY at a wave-uniform base, each lane's source address is free.  Two images:

(a) ROW image.  Per operand four REGIONS of [32 k][256 bytes]: region R holds column groups
    4 R .. 4 R + 3 (A: the 64 columns wave row R >> 1 reads in half-step R & 1; B: the 64 columns
    of wave column R).  A piece is four rows of a region (1 KB); position p of piece q holds row
    4 q + (p >> 4), chunk (p & 15) ^ s(row), s(row) = (row & 7) << 1: the swizzle sits on the SOURCE
    side, sixteen consecutive lanes fetch 256 contiguous bytes (two whole lines).  ds_read_b64_tr_b16
    takes its per-lane addresses 256 bytes (a row) apart; the eight rows of a 32-lane half fall
    into the eight 32-byte windows of the 256-byte bank row.
(b) SUBTILE image.  Today's [32 k][16 columns] subtile per (column group, plane), one DMA
    instruction per subtile: lane p fetches row p >> 1, chunk 4 grp + 2 plane + (p & 1).

Both give every fragment lane today's halfs and both are free of bank conflicts, so the LDS side
does not decide.  The source side does: an instruction of (b) gathers 32-byte segments of 32
different rows, i.e. touches 32 lines of which it uses a quarter each, and every line is fetched by
four different instructions; one of (a) touches 8 lines and uses them whole, as the register-staged
loader does.  (a) is the one built.
"""
ROWS, CHUNKS, PIECE, REGION, IMG = 32, 64, 1024, 8192, 32768
WAVES, WN, MI, NJ = 8, 4, 4, 2
HALVES = [list(range(0, 32)), list(range(32, 64))]        # service groups of ds_read_b64_tr_b16


# ---- today's image (HlLoaderT): what a fragment lane must receive

def today_source(grp, plane, lane, t):
    """(row, chunk of the slab row, byte within the chunk) of the 8 bytes lane `lane` supplies to
    read t (rows 16 t ..) of subtile (grp, plane): byte 8 lane + 512 t of [32 k][32 bytes]."""
    byte = 8 * lane + 512 * t
    return byte // 32, 4 * grp + 2 * plane + (byte % 32) // 16, byte % 16


# ---- the kernel's expressions, layout (a)

def swz(row):
    return (row & 7) << 1


def a_pieces(wave):
    """A is private to a row of waves and a half-step: region 2 wm + h; a wave stages pieces
    wn and wn + 4 of each (q & 1 == wn & 1)."""
    wm, wn = wave // WN, wave % WN
    return [[8 * (2 * wm + h) + wn + 4 * q for q in range(2)] for h in range(2)]


def b_pieces(wave):
    """piece `wave` of every region (q & 1 == wn & 1 again)."""
    return [8 * i + wave for i in range(4)]


def lane_source(wave, piece, lane):
    """(row, chunk of the slab row) lane `lane` of `wave` fetches for `piece`: one per-lane offset
    (row lane >> 4, chunk cs) for all pieces of a wave; the piece's rows and its region's columns
    are a scalar offset."""
    wn = wave % WN
    r4 = lane >> 4
    cs = (lane & 15) ^ ((((wn & 1) << 2) | r4) << 1)
    return 4 * (piece & 7) + r4, 16 * (piece >> 3) + cs


def lane_dest(piece, lane):
    return PIECE * piece + 16 * lane              # M0 = the piece, + 16 bytes per lane


def frag_addr(grp, plane, lane, t):
    """Byte address lane `lane` gives ds_read_b64_tr_b16 for read t of column group grp."""
    row = lane >> 2
    fro = 256 * row + 16 * (((lane >> 1) & 1) ^ swz(row)) + 8 * (lane & 1)
    return REGION * (grp >> 2) + (fro ^ (64 * (grp & 3) + 32 * plane)) + 4096 * t


def a_frag_groups(wave):
    wm = wave // WN
    return [[wm * 2 * MI + hf * MI + i for i in range(MI)] for hf in range(2)]


def b_frag_groups(wave):
    wn = wave % WN
    return [wn * 2 * NJ + j for j in range(2 * NJ)]


def build_image(pieces_of):
    image = {}
    for wave in range(WAVES):
        for piece in pieces_of(wave):
            for lane in range(64):
                dst = lane_dest(piece, lane)
                assert dst not in image
                image[dst] = lane_source(wave, piece, lane)
    return image


def a_pieces_flat(wave):
    return [p for half in a_pieces(wave) for p in half]


IMAGES = {'A': build_image(a_pieces_flat), 'B': build_image(b_pieces)}


def test_every_chunk_of_a_slab_is_written_exactly_once():
    for name, image in IMAGES.items():
        assert sorted(image) == [16 * g for g in range(ROWS * CHUNKS)], name         # dense, 32 KB
        assert sorted(image.values()) == [(r, c) for r in range(ROWS) for c in range(CHUNKS)], name


def test_the_image_fits_two_buffers_in_128_kb():
    assert max(IMAGES['A']) + 16 == IMG and max(IMAGES['B']) + 16 == IMG
    assert 2 * 2 * IMG == 128 * 1024


def test_one_lane_offset_serves_every_piece_of_a_wave():
    for wave in range(WAVES):
        per_lane = set()
        for p in a_pieces_flat(wave) + b_pieces(wave):
            per_lane.add(tuple((lane_source(wave, p, l)[0] - 4 * (p & 7),
                                lane_source(wave, p, l)[1] - 16 * (p >> 3)) for l in range(64)))
        assert len(per_lane) == 1


def test_the_lane_expression_is_the_row_swizzle():
    for wave in range(WAVES):
        for p in a_pieces_flat(wave) + b_pieces(wave):
            for lane in range(64):
                row, c = lane_source(wave, p, lane)
                assert c >> 4 == p >> 3 and (c & 15) == (lane & 15) ^ swz(row)


def test_a_wave_instruction_fetches_eight_whole_lines():
    """16 lanes = 256 contiguous bytes of one row: two 128-byte lines, used whole."""
    for wave in range(WAVES):
        for p in a_pieces_flat(wave) + b_pieces(wave):
            lines = set()
            for r4 in range(4):
                got = [lane_source(wave, p, 16 * r4 + e) for e in range(16)]
                assert {r for r, _ in got} == {4 * (p & 7) + r4}
                assert sorted(c for _, c in got) == list(range(16 * (p >> 3), 16 * (p >> 3) + 16))
                lines |= {(r, c >> 3) for r, c in got}
            assert len(lines) == 8


def test_a_regions_are_private_to_their_wave_row_and_half_step():
    """The ordering rules of the K loop lean on this: the A columns a wave stages for half-step h
    are read by waves of its own row in half-step h only."""
    for wave in range(WAVES):
        wm = wave // WN
        for h in range(2):
            assert {p >> 3 for p in a_pieces(wave)[h]} == {2 * wm + h}
            assert {g >> 2 for g in a_frag_groups(wave)[h]} == {2 * wm + h}
    for region in range(4):
        stagers = {w // WN for w in range(WAVES) for p in a_pieces_flat(w) if p >> 3 == region}
        assert stagers == {region >> 1}


def test_fragment_lanes_receive_what_todays_image_gives_them():
    for name, groups_of in (('A', lambda w: [g for h in a_frag_groups(w) for g in h]),
                            ('B', b_frag_groups)):
        image = IMAGES[name]
        for wave in range(WAVES):
            for grp in groups_of(wave):
                for plane in range(2):
                    for t in range(2):
                        for lane in range(64):
                            row, chunk, byte = today_source(grp, plane, lane, t)
                            addr = frag_addr(grp, plane, lane, t)
                            assert addr % 8 == 0 and 0 <= addr < IMG
                            assert image[addr & ~15] == (row, chunk), (name, grp, plane, lane, t)
                            assert addr % 16 == byte


def _conflicts(addr_of_lane):
    """ds_read_b64_tr_b16: two 32-lane halves, 64 banks of 4 bytes; a lane covers two banks."""
    bad = 0
    for half in HALVES:
        banks = [b for lane in half for b in ((addr_of_lane(lane) // 4) % 64,
                                              (addr_of_lane(lane) // 4 + 1) % 64)]
        bad += len(banks) - len(set(banks))
    return bad


def test_no_half_of_the_transposing_read_shares_a_bank():
    for grp in range(16):
        for plane in range(2):
            for t in range(2):
                assert _conflicts(lambda l: frag_addr(grp, plane, l, t)) == 0
    # the same rows without the source-side swizzle: eight rows on the same four banks
    assert _conflicts(lambda l: 256 * (l >> 2) + 8 * (l & 3)) > 0


def test_rows_and_columns_out_of_range_are_lane_predicates():
    """The scalar offset is outside the descriptor's range check, so the kernel compares: a lane is
    sent out of range (-> zeros in LDS) iff its row is past the reduction range or its column
    group starts past the operand's extent rounded up to a group -- what HlLoaderT.init does."""
    depth, extent, col0 = 8, 300, 256            # K tail of 8, operand of 300 columns, second tile
    for wave in range(WAVES):
        for p in a_pieces_flat(wave) + b_pieces(wave):
            for lane in range(64):
                row, c = lane_source(wave, p, lane)
                r4, cs = lane >> 4, c & 15
                ok = 4 * (p & 7) + r4 < depth and \
                    col0 + 64 * (p >> 3) + 16 * (cs >> 2) < (extent + 15) // 16 * 16
                assert ok == (row < depth and col0 + 16 * (c >> 2) < 304)


# ---- layout (b), on record

def subtile_source(grp, plane, lane):
    return lane >> 1, 4 * grp + 2 * plane + (lane & 1)


def test_subtile_layout_is_todays_image_but_gathers_32_lines_per_instruction():
    for grp in range(16):
        for plane in range(2):
            for lane in range(64):                # M0 = the subtile, + 16 lane = today's store
                row, c = subtile_source(grp, plane, lane)
                assert 16 * lane == row * 32 + (c & 1) * 16
                assert (c >> 1) == 2 * grp + plane
            lines = {(r, c >> 3) for r, c in (subtile_source(grp, plane, l) for l in range(64))}
            assert len(lines) == 32
