"""Host side of the 10-node / 8-node GATHER maps (csrc/gather10.cpp), no device: the crafted meshes of
gather10_meshes.py reach the edges of the chunk records they are meant to reach.  test_gpu_gather10_limits.py
assembles the same meshes on the GPU; these checks keep it honest -- a GPU test of an edge the maps never reach
proves nothing about that edge.

Edges of a chunk record (include/fea_hip.h, feahip_host_gather10_shape):
  - 127 element record slots (7-bit), the slot after the last one the all-zero record;
  - FEA_Q_REGW = 4 list words (8 contributions) per block slot in registers, longer lists read inside the gather;
  - 1 to 7 write-out passes through the K tile (pass 6 is decoded from the header's second word); a row longer than
    half the tile fits no chunk;
  - residual lanes of 2 fdw visits each.
The maps are built in the node numbering a context uses (library ids), so every mesh is looked at in it."""
import numpy as np
import pytest

import feahip
import mesh
import gather10_meshes as gm

Q_MAX_ELEMS = 127
Q_REGW_ENTRIES = 8            # FEA_Q_REGW words of two contributions


def test_shape_reports_a_lattice():
    s = gm.shape(mesh.bar_deck(dims=(2, 4, 2), quadratic=True))
    assert s["ok"] and s["limit"] is None and s["chunks"] >= 2
    assert s["zero_slot"] == Q_MAX_ELEMS                      # the K tile is sized for the element limit
    assert s["tile_blocks"] == (Q_MAX_ELEMS * 31 * 16) // 72 - 1
    assert 1 <= s["min_passes"] <= s["max_passes"] <= 7
    assert gm.shape(gm.hex8_edge_fan(3))["tile_blocks"] == (Q_MAX_ELEMS * 25 * 16) // 72 - 1
    with pytest.raises(feahip.FeaHipError):                     # 4-node elements have maps of their own
        feahip.host_gather10_shape(mesh.bar_deck(dims=(1, 1, 1)).elements, 8)


@pytest.mark.parametrize("make", [gm.tet10_edge_fan, gm.hex8_edge_fan], ids=["tet10", "hex8"])
def test_edge_fan_lists_leave_the_registers_past_eight_elements(make):
    """k elements around one axis edge: the edge's block (and, for TET10, its mid-side node's) gets one contribution
    per element.  Eight fit the four register words; the ninth is read from memory inside the gather phase."""
    s8, s9, s12 = gm.shape(make(8)), gm.shape(make(9)), gm.shape(make(12))
    assert s8["ok"] and s8["longest_list"] == 8 and s8["chunks_with_long_lists"] == 0
    assert s9["ok"] and s9["longest_list"] == 9 and s9["chunks_with_long_lists"] >= 1
    assert s12["ok"] and s12["longest_list"] == 12 and s12["chunks_with_long_lists"] >= 1


def test_tet10_hub_bracket_is_the_element_limit():
    """A quadratic hub grown one element at a time: 127 elements around one node still build -- its chunk fills all
    127 record slots, the all-zero record right after the last -- and the 128th is refused for its element count
    (the hub's row is still far from half the K tile)."""
    ok, over = gm.shape(gm.tet10_node_hub(127)), gm.shape(gm.tet10_node_hub(128))
    assert ok["ok"] and ok["max_elems"] == Q_MAX_ELEMS and ok["chunks_at_elem_limit"] >= 1
    assert ok["zero_slot"] == Q_MAX_ELEMS
    assert ok["chunks_with_long_lists"] >= 1 and ok["longest_list"] > Q_REGW_ENTRIES
    assert not over["ok"] and over["limit"] == "elements" and over["limit_row"] >= 0
    deck = gm.tet10_node_hub(128)
    rowlen = len(np.unique(deck.elements[np.any(deck.elements == 0, axis=1)]))
    assert rowlen <= ok["tile_blocks"] // 2                    # row length is not what binds here


def test_hex8_hub_bracket_is_the_row_length():
    """Bricks around one axis edge, grown one at a time (open fan): the axis node's row reaches half the K tile
    (352 blocks) at 87 bricks, long before the 127 records -- row length is the limit that binds."""
    ok, over = gm.shape(gm.hex8_edge_fan(87, closed=False)), gm.shape(gm.hex8_edge_fan(88, closed=False))
    assert ok["ok"] and over["limit"] == "row length" and not over["ok"]
    assert ok["max_elems"] == 87 < Q_MAX_ELEMS
    deck = gm.hex8_edge_fan(87, closed=False)
    rowlen = len(np.unique(deck.elements[np.any(deck.elements == 0, axis=1)]))
    assert rowlen == ok["tile_blocks"] // 2                    # the longest row that fits
    assert ok["longest_list"] == 87 and ok["chunks_with_long_lists"] >= 1


@pytest.mark.parametrize("npe", [10, 8])
def test_fan_welded_into_a_lattice_overflows_between_ordinary_chunks(npe):
    """A 12-element fan on an edge in the middle of a lattice: the edge's block list (the lattice's contributions and
    the fan's) outgrows the registers in a chunk that has ordinary chunks before and after it."""
    deck = gm.tet_lattice_with_fan((3, 8, 3), 12) if npe == 10 else gm.hex_lattice_with_fan((4, 12, 4), 12)
    s = gm.shape(deck)
    assert s["ok"] and s["longest_list"] > 12
    assert s["chunks_with_long_lists"] < s["chunks"]
    assert 0 < s["first_long_list_chunk"] < s["chunks"] - 1


@pytest.mark.parametrize("npe", [10, 8])
def test_lattice_reaches_two_words_per_residual_lane_and_many_nodes(npe):
    """The default chunks of a lattice: more visits than 128 lanes of one word (fdw = 2); with a fan welded in (or a
    large fan alone, for bricks), more nodes than the 240 an 8-bit chunk-local node id would number -- the 10-node
    records name elements, not nodes, so no node limit applies and none may be imposed by accident."""
    deck = mesh.bar_deck(dims=(3, 8, 3), quadratic=True) if npe == 10 else gm.deck_of(*mesh.hex_block(6, 12, 6), 8)
    s = gm.shape(deck)
    assert s["ok"] and s["max_fdw"] >= 2 and s["max_rows"] >= 48
    crowded = gm.tet_lattice_with_fan((3, 8, 3), 12) if npe == 10 else gm.hex8_edge_fan(87, closed=False)
    s = gm.shape(crowded)
    assert s["ok"] and s["max_nodes"] >= 240


@pytest.mark.parametrize("case", ["tet10", "hex8"])
def test_element_knob_sets_the_write_out_passes(case, monkeypatch):
    """FEAHIP_GATHER10_ELEMS shrinks the chunks and the K tile with them.  The chunk cut bounds a chunk's blocks by
    five tiles, but the passes take whole rows of up to half a tile each, so a tile can go out nearly half empty: two
    TET10 sharing a face (rows of 14 and 10 blocks, 164 blocks in all) under a 33-block tile, or three bricks in a row
    (rows of 12 and 8, 160 blocks) under a 26-block tile, need all seven passes.  The default gives one pass.  Below
    the longest row's half tile nothing builds -- the row length binds."""
    deck = gm.tet10_face_pair() if case == "tet10" else gm.hex8_row_of_three()
    monkeypatch.setenv("FEAHIP_GATHER10_ELEMS", "5")
    s = gm.shape(deck)
    assert s["ok"] and s["max_passes"] == 7
    assert s["tile_blocks"] == (33 if case == "tet10" else 26)
    monkeypatch.setenv("FEAHIP_GATHER10_ELEMS", "4")
    s = gm.shape(deck)
    assert not s["ok"] and s["limit"] == "row length"
    assert s["tile_blocks"] == (26 if case == "tet10" else 21)     # reported also when the maps do not build
    monkeypatch.setenv("FEAHIP_GATHER10_ELEMS", "127")
    s = gm.shape(deck)
    assert s["ok"] and s["max_passes"] == 1


def test_bricks_have_no_cache_table_rule():
    """The shape-gradient table read through the cache serves rules of more than 8 points.  Bricks have the 8-point
    rule only: a 27-point brick rule is refused, so the 8-node cache-table kernels are never launched."""
    with pytest.raises(feahip.FeaHipError, match="27 Gauss points"):
        feahip.element_tables(feahip.HEXAHEDRA8, 27)
    feahip.element_tables(feahip.TETRAHEDRA10, 27)


def test_tet4_overflow_chunk_follows_a_repeated_chunk():
    """4-node maps: a 50-tetrahedron fan welded into a long TET4 lattice.  The chunk whose lists outgrow the
    registers (block and diagonal lists) comes right after a chunk that repeats its predecessor's map words -- the
    chunk the kernel runs with the words it kept in registers -- so the overflow chunk must load its own."""
    deck = gm.tet_lattice_with_fan((3, 60, 3), 50, quadratic_=False)
    flags = feahip.host_gather_chunks(gm.library_elements(deck), len(deck.nodes))
    over = np.nonzero(flags & 6)[0]
    assert len(over) >= 1 and np.all(flags[over] & 2) and np.any(flags[over] & 4)
    assert any(p >= 2 and flags[p - 2] & 1 for p in over)       # chunk p - 1 repeats chunk p - 2's words
    assert 0 < over[0] < len(flags) - 1


def test_row_knob_is_honoured(monkeypatch):
    deck = mesh.bar_deck(dims=(3, 8, 3), quadratic=True)
    monkeypatch.setenv("FEAHIP_GATHER10_ROWS", "16")
    s = gm.shape(deck)
    assert s["ok"] and s["max_rows"] == 16
    monkeypatch.setenv("FEAHIP_GATHER10_ALPHA", "0")
    assert gm.shape(deck)["chunks"] >= s["chunks"]


def test_shape_agrees_with_gather_stats():
    """The two host views of the 10-node maps agree on the chunks of a renumbered, jittered deck (test_gpu_gather10_limits.py
    checks the chunk count against what a context reports it built)."""
    deck = mesh.jitter_permute(mesh.bar_deck(dims=(2, 6, 2), quadratic=True))
    ids, renumbered = feahip.host_numbering(deck.elements, deck.nodes)
    assert renumbered
    s = gm.shape(deck)
    st, _ = feahip.host_gather_stats(ids[deck.elements], len(deck.nodes))
    assert s["ok"] and s["chunks"] == st["chunks"]
