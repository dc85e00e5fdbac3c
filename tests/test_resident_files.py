"""The small LAST corpora of the resident-dataset tests are, byte for byte, what those tests wrote before they shared a writer
(tests/_resident_files.py): the seeds were chosen so that the boxes, rasters and outlines hit what their comments say.  The digests
were recorded by running each module's own `files` fixture as it stood before the writer was shared.  No GPU call."""
import hashlib
import importlib
import os

import pytest

import _resident_files as rf

# module -> sha256 of each file its corpus(d) writes, in load order
DIGESTS = {
    "multi": [("f0_1_12305.last", "3870611dd9f201959b079c30d3eb5bf80c29d9190bb9df41acd56e48586ccac3"),
              ("f1_3_4096.last", "5faa31b435bde0a5521cb11b245c5cdd01501cedf838e26aeef9c62cc85a9224"),
              ("f2_6_100.last", "6ffb0c9731ca05c62b4c3c628924c5e2f76d0e9eb01186c8cb9c675e4872fcbe"),
              ("f3_1_0.last", "f19a7f13eb115fa2ca1e94eeb494b5c8298dcc1e98ec93d4d34b5ac37b989988"),
              ("f4_3_8197.last", "1ba1fd12f2d905ccca3b429cab8518470c19b6a35ca2f1d112e8518a99951e80")],
    "class_hist": [("f0_1_12305.last", "24f21ae16c00fb732fcfb8b67332bfee61251c284ecf7aa0bd9c4955e844ace4"),
                   ("f1_3_4096.last", "560db46162c488b2297816e82ba3513ba19ee629e715343a02e5456c922410dd"),
                   ("f2_6_100.last", "4942e3e03cf071bff93aa10d19c5991ca7b1a7865d84d93f7849def07617ab65"),
                   ("f3_1_0.last", "f19a7f13eb115fa2ca1e94eeb494b5c8298dcc1e98ec93d4d34b5ac37b989988"),
                   ("f4_3_8197.last", "d60ab377ae975930c740fe8664556a1c5e1f5aecb5b9ab4b68be6f6641081ad8")],
    "raster": [("f0_1_12305.last", "16ffff97b7d640e7834913473757b1fda82cf6f4e874f65447ca61a134193080"),
               ("f1_3_4096.last", "fd247d1dbc5ee0f9958fc9f5369f5e4c3a3e52d4a21d6a0ebd9d80ecde603da1"),
               ("f2_6_100.last", "22933de860182a6d96557e0778d582d9c1f7d3b84357a206072596d2dcb1feb0"),
               ("f3_1_0.last", "f19a7f13eb115fa2ca1e94eeb494b5c8298dcc1e98ec93d4d34b5ac37b989988"),
               ("f4_3_8197.last", "e6a71f473123e4c3467ce82824e0dcc5efe040920496b81ffb254ccc186e164f")],
    "zrange": [("f0_1_12305.last", "16ffff97b7d640e7834913473757b1fda82cf6f4e874f65447ca61a134193080"),
               ("f1_3_4096.last", "fd247d1dbc5ee0f9958fc9f5369f5e4c3a3e52d4a21d6a0ebd9d80ecde603da1"),
               ("f2_6_100.last", "22933de860182a6d96557e0778d582d9c1f7d3b84357a206072596d2dcb1feb0"),
               ("f3_1_0.last", "f19a7f13eb115fa2ca1e94eeb494b5c8298dcc1e98ec93d4d34b5ac37b989988"),
               ("f4_3_8197.last", "e6a71f473123e4c3467ce82824e0dcc5efe040920496b81ffb254ccc186e164f")],
    "zrange_flat": [("f0_3_4096.last", "fcc1d0cfb30ec4282868b4a3c80769f2d8ccef871c3e61ce92e189d402f3a11a"),
                    ("f1_1_600.last", "3121a731fec8a8de42adcdd71761ed8edf75d5e83db7287e61711ce07f0a4fc6")],
    "zrange_shared": [("f0_1_4105.last", "0ea116935ca1e36f855d862c4795c0dd9770d7521db08c915887f220c3876469"),
                      ("f1_3_700.last", "0f21ba2431e45358ecfc03f20e23f6f2858ef460c859d7372e71a69819f0ab66"),
                      ("f2_3_8192.last", "233ab0679b3072707a46e92bef78b96663647c48c2dd4a03687d3266d692cd5a")],
    "polygon": [("f0_1_12305.last", "16ffff97b7d640e7834913473757b1fda82cf6f4e874f65447ca61a134193080"),
                ("f1_3_4096.last", "fd247d1dbc5ee0f9958fc9f5369f5e4c3a3e52d4a21d6a0ebd9d80ecde603da1"),
                ("f2_6_100.last", "22933de860182a6d96557e0778d582d9c1f7d3b84357a206072596d2dcb1feb0"),
                ("f3_1_0.last", "f19a7f13eb115fa2ca1e94eeb494b5c8298dcc1e98ec93d4d34b5ac37b989988"),
                ("f4_3_8197.last", "e6a71f473123e4c3467ce82824e0dcc5efe040920496b81ffb254ccc186e164f")],
    "time_hist": [("f0_1_12305.last", "b5d2d72cba1944d35877aedd016321c67d03283217853789a1882c6849d8cb35"),
                  ("f1_6_4096.last", "9fdcc45123c42dd385d1de455a477de5d4e27b6e2b174e55b0382cc60a1a2ca4"),
                  ("f2_3_100.last", "8857917bb1c1d3522f8128ef2ddaeae0568eb16de8af22b1fdf9ced8623d48b5"),
                  ("f3_1_0.last", "f19a7f13eb115fa2ca1e94eeb494b5c8298dcc1e98ec93d4d34b5ac37b989988"),
                  ("f4_6_513.last", "b8b10088a48b280d7161ba448c3971afc9a35b6322a74a805243d6cf02aef1b8"),
                  ("f5_1_8197.last", "5e0d109040efd2fdb15509118fc5b2c04d2f3258780a5c5f36ce388ee42f9c5f")],
}
# the two extra corpora of test_gpu_resident_zrange.py: (specs, seed)
ZRANGE_EXTRA = {"zrange_flat": ([(3, 4096, rf.ISO, (0.0, 0.0, 0.0)), (1, 600, (0.01, 0.01, 0.0), (200.0, 0.0, 1.0))], 970),
                "zrange_shared": ([(1, 4096 + 9, (0.01, 0.02, 0.05), (0.0, 0.0, 7.5)), (3, 700, rf.ISO, (1.0, -1.0, 0.0)),
                                   (3, 2 * 4096, (0.02, 0.01, 0.05), (10.0, -10.0, 7.5))], 980)}


def digests(paths):
    return [(os.path.basename(p), hashlib.sha256(open(p, "rb").read()).hexdigest()) for p in paths]


@pytest.mark.parametrize("name", list(DIGESTS))
def test_the_corpus_is_what_it_was(tmp_path, name):
    if name in ZRANGE_EXTRA:
        paths, held = rf.write_files(tmp_path, *ZRANGE_EXTRA[name])
    else:
        paths, held = importlib.import_module("test_gpu_resident_" + name).corpus(tmp_path)
    assert digests(paths) == DIGESTS[name]
    for p, h in zip(paths, held):  # what the tests hold of a file is what is on disk
        assert h.image.tobytes() == open(p, "rb").read() and len(h.xyz) == len(h.cls) == len(h.t)


def test_the_lying_file_lies_about_its_x_maximum(tmp_path):
    _, held = rf.write_files(tmp_path, rf.FIVE_FILES, 950, rf.LYING)
    h = held[rf.LYING]
    assert h.hmax[0] == rf.LYING_XMAX and rf.meets(h, ((260.0, -40.0, -8.0), (290.0, 40.0, 8.0)))
    assert not rf.meets(h, ((320.0, -50.0, -10.0), (340.0, 50.0, 10.0)))  # its points are there, its header is not
