"""nn_ops.WeightShadows: the 16-bit weight shadows of a module have ONE owner, and they go when it goes (host tensors: plain torch copies)."""
import gc
import weakref

import torch

from cosa_amd import nn_ops


def test_shadows_die_with_their_owner_and_a_new_module_resolves_to_nothing():
    """build an owner for a small module, drop module and owner, collect: a parameter and its 16-bit copy are both gone (process-global
    id-keyed maps with strong references used to keep both until the process ended); then no parameter of a second module -- whose tensors
    may reuse the ids of the first one's -- resolves to an entry before its own owner is built"""
    lin = torch.nn.Linear(8, 8)
    sh = nn_ops.ensure_shadows(lin)
    assert sh is lin.__dict__["_weight_shadows"] and nn_ops.ensure_shadows(lin) is sh
    assert all(torch.equal(nn_ops.shadow_of(p), p.detach().to(torch.bfloat16)) for p in lin.parameters())
    assert nn_ops.shadow_entry(lin.weight, torch.float16) is None and nn_ops.shadow_entry(lin.weight, torch.bfloat16)[1] is None
    w_param, w_copy = weakref.ref(lin.weight), weakref.ref(nn_ops.shadow_of(lin.weight))
    del lin, sh
    gc.collect()
    assert w_param() is None and w_copy() is None
    assert len(nn_ops._owner_of) == 0
    for _ in range(8):                      # (several: the allocator hands the freed addresses out again)
        other = torch.nn.Linear(8, 8)
        assert all(nn_ops.shadow_of(p) is None and nn_ops.shadow_entry(p) is None for p in other.parameters())
        assert nn_ops.cast_param(other.weight.detach(), torch.bfloat16).dtype == torch.bfloat16
    own = nn_ops.ShadowSet(other)
    assert all(nn_ops.shadow_of(p) is s for p, s in zip(other.parameters(), own.shadows))


def test_refresh_leaves_optimizer_owned_copies_alone_unless_forced_and_an_owned_set_is_not_replaced():
    lin = torch.nn.Linear(8, 8)
    sh = nn_ops.ensure_shadows(lin)
    with torch.no_grad():
        lin.weight.add_(1.0)
    with nn_ops.shadows_fresh(lin):         # nested entry points skip their refresh
        nn_ops.ensure_shadows(lin)
        assert not torch.equal(sh.shadows[0], lin.weight.detach().to(torch.bfloat16))
    nn_ops.ensure_shadows(lin)
    assert torch.equal(sh.shadows[0], lin.weight.detach().to(torch.bfloat16))
    sh.optimizer_owned = True
    with torch.no_grad():
        lin.weight.add_(1.0)
    nn_ops.ensure_shadows(lin)
    sh.refresh()
    assert not torch.equal(sh.shadows[0], lin.weight.detach().to(torch.bfloat16))
    sh.refresh(force=True)
    assert torch.equal(sh.shadows[0], lin.weight.detach().to(torch.bfloat16))
    try:
        nn_ops.ensure_shadows(lin, torch.float16)
    except RuntimeError as e:
        assert "owned by a CoSATrainer" in str(e)
    else:
        raise AssertionError("an optimizer-owned shadow set was replaced")
    import copy
    assert "_weight_shadows" not in {k for k, v in copy.deepcopy(lin).__dict__.items() if v is not None}     # a copy starts without an owner
