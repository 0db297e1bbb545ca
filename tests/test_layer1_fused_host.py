"""Host side of the one-launch layer 1: who asks the library to keep the layer-1 means (sage_model_t.keep_means, ABI 8)."""
import os
import re
import types

import torch

from sage355 import native
from sage355.engine import TwoHopEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_struct_ends_with_keep_means_as_the_header_does():
    header = open(os.path.join(REPO, "include", "sage355.h")).read()
    body = header[header.index("typedef struct {\n    /* Each Encoder holds"):header.index("} sage_model_t;")]
    fields = re.findall(r"^\s+(?:const\s+)?[A-Za-z_0-9]+\*?\s+\*?([a-z_0-9]+(?:\s*,\s*[a-z_0-9]+)*);", body, re.M)
    names = [n.strip() for f in fields for n in f.split(",")]
    assert names == [n for n, _ in native.Model._fields_], "native.Model out of step with sage_model_t"
    assert names[-1] == "keep_means" and native.ABI_VERSION >= 8


def test_who_wants_the_means():
    w = torch.zeros(2, 2)
    wg = torch.zeros(2, 2, requires_grad=True)
    eng = types.SimpleNamespace(keep_means=False, w1=w, w2=w)
    assert not TwoHopEngine._wants_means(eng)                       # serving: RolePipeline, TwoHopEngine.forward / replay / capture
    eng.keep_means = True                                           # EngineTrainer and autograd._TwoHop set it
    assert TwoHopEngine._wants_means(eng)
    eng = types.SimpleNamespace(keep_means=False, w1=wg, w2=w)
    assert TwoHopEngine._wants_means(eng)                           # a forward under grad mode on weights that train
    with torch.no_grad():
        assert not TwoHopEngine._wants_means(eng)


def test_training_entry_points_set_keep_means():
    src = os.path.join(REPO, "graphsage-simple_amd", "sage355")
    assert "self.engine.keep_means = True" in open(os.path.join(src, "train.py")).read()
    assert "engine.keep_means = True" in open(os.path.join(src, "autograd.py")).read()
    pipe = open(os.path.join(src, "engine.py")).read()
    pipe = pipe[pipe.index("class RolePipeline"):]
    assert "keep_means" not in pipe                                 # the pipeline never asks for the means
