"""stream.prepare_phase2_plan is host arithmetic: which prefix of which vector is loaded from where, how the sections tile every
phase1radix2m{k} file, the order of the work and the device memory it needs.  Powers 0, 1, 4 and 28 with every degree, power 28 with one."""
import pytest

PLANS = [(0, None), (1, None), (4, None), (28, None), (28, [20])]


@pytest.mark.parametrize("power,degrees", PLANS)
def test_sections_tile_every_file_in_the_radix_order(zk, power, degrees):
    plan = zk.prepare_phase2_plan(power, degrees)
    assert list(plan.files) == (list(range(power + 1)) if degrees is None else degrees) == list(plan.degrees)
    for k, f in plan.files.items():
        m = 1 << k
        assert f.size == 256 + 320 * m + 64 * (m - 1)
        assert [s.name for s in f.sections.values()] == [name for name, _, _ in zk.ceremony._RADIX_FIELDS] == list(f.sections)
        off = 0
        for (name, g, cnt), s in zip(zk.ceremony._RADIX_FIELDS, f.sections.values()):
            assert (s.group, s.count, s.offset) == (g, cnt(m), off), (k, name)
            off += s.count * 64 * g
        assert off == f.size


@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("power,degrees", PLANS)
def test_loads_are_the_prefixes_at_the_accumulators_offsets(zk, power, degrees, compressed):
    plan = zk.prepare_phase2_plan(power, degrees, compressed)
    kmax = power if degrees is None else max(degrees)
    assert plan.kmax == kmax
    layout, body = zk.ceremony.accumulator_layout(power, compressed)
    assert plan.input_size == (zk.stream.response_size(power) if compressed else zk.stream.challenge_size(power))
    assert plan.input_size == body + (zk.keys.PUBLIC_KEY_SIZE if compressed else 0)
    assert list(plan.loads) == [name for name, _, _, _ in layout]
    for name, g, cnt, off in layout:
        ld = plan.loads[name]
        want = {"tau_g1": (2 << kmax) - 1, "beta_g2": 1}.get(name, 1 << kmax)
        assert (ld.vector, ld.group, ld.offset) == (name, g, off)
        assert ld.count == want <= cnt                                # never more than the file holds
        assert off + ld.count * (32 if compressed else 64) * g <= body


@pytest.mark.parametrize("power,degrees", PLANS)
def test_the_order_is_vector_major_and_loads_each_vector_once(zk, power, degrees):
    plan = zk.prepare_phase2_plan(power, degrees)
    loads = [s[1] for s in plan.order if s[0] == "load"]
    assert loads == ["tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2"]
    resident, written = None, set()
    for step in plan.order:
        if step[0] == "load":
            assert resident is None                                   # one vector at a time
            resident = step[1]
        elif step[0] == "free":
            assert resident == step[1]
            resident = None
        elif step[0] == "ifft":
            assert resident == step[1]
            written.add((step[2], step[3]))
        elif step[0] == "h":
            assert resident == "tau_g1" and step[1] > 0
            written.add((step[1], "h"))
        else:
            assert step[0] == "head" and resident == step[1]
            written |= {(k, step[1]) for k in plan.degrees}
    assert resident is None
    # every section of every file is written exactly by these steps (h of degree 0 is empty)
    assert written == {(k, name) for k in plan.degrees for name, _, _ in zk.ceremony._RADIX_FIELDS if not (name == "h" and k == 0)}


def test_degrees_are_checked_and_collapse(zk):
    plan = zk.prepare_phase2_plan(4, [3, 1, 3, 1])
    assert plan.degrees == (1, 3) and list(plan.files) == [1, 3] and plan.kmax == 3
    for bad in ([-1], [5], [2.0], ["2"], [], [True], [1, 9]):
        with pytest.raises(ValueError):
            zk.prepare_phase2_plan(4, bad)
    for power in (-1, 29, 2.5):
        with pytest.raises(ValueError):
            zk.prepare_phase2_plan(power)


def test_device_bytes_grows_with_the_degree_and_the_piece(zk):
    pieces = (1, 3, 1 << 10, 1 << 18, 1 << 22)
    for piece in pieces + (0,):
        sizes = [zk.prepare_phase2_plan(28, [k]).device_bytes(piece) for k in range(29)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), piece
    for k in (0, 4, 20, 28):
        plan = zk.prepare_phase2_plan(28, [k])
        sizes = [plan.device_bytes(p) for p in pieces]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), k
        assert plan.device_bytes(0) == plan.device_bytes(zk.lib.POINTS_PIECE)
        # one vector, its work buffer and one transform's scratch: the G2 vector at least, and nothing index-shaped on top (72 B per output
        # is what the sparse product's indices and coefficients cost)
        n = 1 << k
        assert plan.device_bytes(0) >= 2 * 128 * n
        assert plan.device_bytes(1) <= (2 * 128 + 224 + 64 + 16 + 8 * 368 + 1) * n * 33 // 32 + 4096   # (1 / 32: the runtime's allowance)
    # the same degree costs the same from a larger file
    assert zk.prepare_phase2_plan(28, [20]).device_bytes() == zk.prepare_phase2_plan(20).device_bytes()
