"""The meshes of tests/rowloop_cases.py reach the limits of the row loop's tile that they name (host only): every entry
of LIMITS satisfies its predicate on the chunk table restated from pattern.cpp's rule, none is renumbered by the library,
and together they reach every shape of SHAPES.  A change of the chunk rule that moves a shape fails here, by name."""
import numpy as np
import pytest

import rowloop_cases as rc
from explicit_reference import hub_fan
from pcg_cases import CHUNK_BLOCKS, CHUNK_ROWS


@pytest.mark.parametrize("name", list(rc.LIMITS))
def test_every_entry_reaches_its_limit(name):
    make, reaches = rc.LIMITS[name]
    deck = make()
    table = rc.chunk_table(deck)
    assert not rc.renumbered(deck), f"{name}: the library renumbers this mesh, deck ids are no longer library ids"
    assert len(deck.nodes) <= 255
    rows = [r for r0, r1, _, _ in table for r in (r0, r1)]
    assert rows[0] == 0 and rows[-1] == len(deck.nodes) and rows[1:-1:2] == rows[2::2]
    assert all(r1 - r0 <= CHUNK_ROWS and (nb <= CHUNK_BLOCKS or r1 - r0 == 1) for r0, r1, _, nb in table)
    assert reaches(deck, table), f"{name} no longer reaches its limit: chunks (rows, b0, nb) {sorted(rc.shapes(table), key=lambda s: s[1])}"


def test_together_the_entries_reach_every_shape():
    tables = {name: rc.chunk_table(make()) for name, (make, _) in rc.LIMITS.items()}
    lost = [shape for shape, holds in rc.SHAPES.items() if not any(holds(t) for t in tables.values())]
    assert not lost, f"no mesh of LIMITS reaches: {lost}"
    for shape, holds in rc.SHAPES.items():
        print(shape, "<-", [n for n, t in tables.items() if holds(t)])


def test_the_last_staged_piece_belongs_to_lane_zero_of_a_full_tile_at_an_odd_block():
    """np == 577 exactly when nb == 128 and b0 is odd; 576 = 9 * 64 pieces go to the nine full rounds of the wave."""
    assert rc.NPMAX == 577
    for b0 in range(0, 6):
        for nb in range(1, CHUNK_BLOCKS + 1):
            assert (rc.staged_pieces(b0, nb) == rc.NPMAX) == (nb == CHUNK_BLOCKS and b0 % 2 == 1)
            assert rc.staged_pieces(b0, nb) <= rc.NPMAX


def test_the_hub_row_of_hub_fan_has_spokes_plus_two_blocks():
    for spokes in (22, 150):
        table = rc.chunk_table(hub_fan(spokes))
        assert table[0][:2] == (0, 1) or spokes + 2 <= CHUNK_BLOCKS
        assert rc.spmv_chunks(hub_fan(spokes))[1][0] == set(range(spokes + 2))
    assert rc.chunk_table(hub_fan(150))[0] == (0, 1, 0, 152)               # still a long row


def test_isolated_nodes_are_rows_of_one_block():
    deck = rc.LIMITS["hub29_hub_ring_pole_iso2"][0]()
    used = np.unique(deck.elements)
    iso = np.setdiff1d(np.arange(len(deck.nodes)), used)
    assert list(iso) == [31, 32]
    nbr = rc.spmv_chunks(deck)[1]
    assert all(nbr[a] == {a} for a in iso)
