"""The host helpers the frozen networks' wrappers share (n3dt/_host.py), as far as they run without a GPU: the state-dict mechanics
with their exact error sentences, for a made-up two-key table, and the chunk loop."""
import pytest
import torch

from n3dt._host import chunks, only_keys, open_state_dict, take

WHO = "load_toy"
TABLE = {"a.weight": (2, 3), "a.bias": (2,)}


def toy():
    return {"a.weight": torch.zeros(2, 3), "a.bias": torch.ones(2)}


def test_open_state_dict_refuses_what_is_no_dict_in_the_callers_words():
    with pytest.raises(TypeError) as e:
        open_state_dict(WHO, [1, 2])
    assert str(e.value) == "load_toy: expected a state dict or a path, got list"
    with pytest.raises(TypeError) as e:
        open_state_dict(WHO, "toy.pth", paths=False)  # a path is not opened
    assert str(e.value) == "load_toy: expected a state dict, got str"
    with pytest.raises(TypeError) as e:
        open_state_dict(WHO, 3, expected="a toy dict or a path to one")
    assert str(e.value) == "load_toy: expected a toy dict or a path to one, got int"


def test_open_state_dict_opens_a_path_unwraps_and_strips(tmp_path):
    sd = toy()
    assert open_state_dict(WHO, sd) is sd
    assert open_state_dict(WHO, {"state_dict": sd, "epoch": 3}, unwrap=("net", "state_dict")) is sd
    assert open_state_dict(WHO, {"state_dict": 3}, unwrap=("state_dict",)) == {"state_dict": 3}  # no dict under the name: left alone
    torch.save({"net": sd}, tmp_path / "toy.pth")
    for path in (tmp_path / "toy.pth", str(tmp_path / "toy.pth")):
        got = open_state_dict(WHO, path, unwrap=("net",))
        assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    got = open_state_dict(WHO, {"module.a.weight": 1, "a.module.bias": 2, 7: 3}, strip_module=True)
    assert got == {"a.weight": 1, "a.module.bias": 2, 7: 3}  # a leading `module.` only


def test_take_refuses_a_missing_key_and_a_wrong_shape_with_the_key():
    sd = toy()
    with pytest.raises(KeyError) as e:
        take(WHO, {"a.weight": sd["a.weight"]}, "a.bias", TABLE["a.bias"])
    assert e.value.args[0] == "load_toy: the state dict has no key 'a.bias'"
    with pytest.raises(KeyError) as e:
        take(WHO, {}, "a.bias", TABLE["a.bias"], alt_keys=("b.bias", "c.bias"))
    assert e.value.args[0] == "load_toy: the state dict has no key 'a.bias' (nor 'b.bias', 'c.bias')"
    with pytest.raises(ValueError) as e:
        take(WHO, {"a.weight": torch.zeros(3, 2)}, "a.weight", TABLE["a.weight"])
    assert str(e.value) == "load_toy: 'a.weight' has shape (3, 2), expected (2, 3)"
    with pytest.raises(ValueError) as e:
        take(WHO, {"a.bias": [0.0, 1.0]}, "a.bias", [(1, 2, 1, 1), (2,)])
    assert str(e.value) == "load_toy: 'a.bias' has shape list, expected (1, 2, 1, 1)"
    with pytest.raises(KeyError) as e:
        only_keys(WHO, {"a.weight": 0, "a.extra": 1}, TABLE)
    assert e.value.args[0] == "load_toy: unexpected key 'a.extra'"
    only_keys(WHO, sd, TABLE)


def test_take_gives_the_callers_tensor_detached_and_alt_keys_pick_the_first_name_present():
    sd = toy()
    sd["a.weight"].requires_grad_(True)
    w = take(WHO, sd, "a.weight", TABLE["a.weight"])
    assert not w.requires_grad and w.data_ptr() == sd["a.weight"].data_ptr() and w.float() is w
    sd["a.bias"].add_(1)  # the counter the caches watch is the caller's
    assert take(WHO, sd, "a.bias", [(1, 2), (2,)])._version == sd["a.bias"]._version == 1
    old, new, newer = torch.full((2,), 1.0), torch.full((2,), 2.0), torch.full((2,), 3.0)
    assert torch.equal(take(WHO, {"old": old, "new": new}, "new", (2,), alt_keys=("old",)), new)     # the key itself first
    assert torch.equal(take(WHO, {"old": old, "newer": newer}, "new", (2,), alt_keys=("old", "newer")), old)
    assert torch.equal(take(WHO, {"newer": newer}, "new", (2,), alt_keys=("old", "newer")), newer)
    with pytest.raises(ValueError) as e:  # the name that was found is the one refused
        take(WHO, {"old": torch.zeros(3)}, "new", (2,), alt_keys=("old",))
    assert str(e.value) == "load_toy: 'old' has shape (3,), expected (2,)"


@pytest.mark.parametrize("n,cap,chunk", [(1, 1, None), (5, 2, None), (5, 8, 3), (7, 3, 0)])
def test_chunks_cover_n_exactly(n, cap, chunk):
    got = list(chunks(n, cap, chunk))
    limit = cap if chunk is None else max(1, min(cap, chunk))  # chunk = 0 clamps to 1
    at = 0
    for i, m in got:
        assert i == at and 1 <= m <= limit
        at += m
    assert at == n
    assert len(got) == -(-n // limit)  # no call is shorter than it has to be
