"""Guided decoding without a GPU: the pattern compiler (models/guided.py)
against ``re.fullmatch`` and a brute-force token walk, its refusals, the NumPy
emulation of ``ops.guide_`` over several steps, request parsing and the eager
engine's refusal. Every comparison is exact."""
import itertools
import json
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd.models import guided
from p2p_llm_tunnel_amd.models.guided import compile_dfa, compile_guide
from p2p_llm_tunnel_amd.models.server import Engine, Request, SamplingError, guided_params, sampling_params
from p2p_llm_tunnel_amd.utils import guide_ref
from tests.guided_cases import brute_table, completion, random_case, synthetic_vocab

# (pattern, alphabet): every string up to length 6 over the alphabet is tried.
PATTERNS = [
    (r"(yes|no|maybe)", "yesnomab"[:5] + "m"),          # alternation
    (r"a(b|c(d|e)*)+f?", "abcdf"),                      # nested groups
    (r"[0-9]{3}-[0-9]{4}", "01-9"),                     # counted repeats
    (r"-?[1-9][0-9]*(\.[0-9]+)?", "-019."),
    (r"(?:ab){,2}c{2,}|b{1,3}", "abc"),
    (r"[^ab]c{2,3}", "abcé\n"),                         # negated class: a whole character, newline included
    (r"[^\d\s]+x", "1 xé"),
    (r"\d+\s\w*[\]\-a]", "1 a]-_"),                     # escapes
    (r"\D\W?\S", "1a é"),
    (r"\x41\t\.\\\|", "A\t.\\|"),
    (r"é+a|日", "éa日b"),                                # non-ASCII literals
    (r".{1,2}b", "ébc\n"),                              # . over a two-byte character, never a newline
    (r"a{2}|{|a{,}", "a{,}"),                           # braces that are no quantifier are literals
]


def test_dfa_agrees_with_re_fullmatch():
    for pattern, alphabet in PATTERNS:
        trans, accept = compile_dfa("regex", pattern)
        want = re.compile(pattern, re.ASCII)
        enc = {c: c.encode() for c in alphabet}
        for n in range(7):
            for tup in itertools.product(alphabet, repeat=n):
                s = 0
                for b in b"".join(enc[c] for c in tup):
                    s = trans[s, b]
                    if s < 0:
                        break
                got = s >= 0 and bool(accept[s])
                assert got == (want.fullmatch("".join(tup)) is not None), (pattern, "".join(tup))
        # trimmed: from every state an accepting one is reachable
        live = accept.copy()
        for _ in range(len(accept)):
            live |= ((trans >= 0) & live[np.maximum(trans, 0)]).any(axis=1)
        assert live.all(), pattern


def test_dfa_is_minimal_and_canonical():
    """State counts of languages whose minimal DFA is known (a dead state is not counted: there is none), and
    spellings of one language give the same arrays, which is what lets their tables share one residency."""
    for pattern, states in ((r"[0-9]{3}-[0-9]{4}", 9), (r"(a|b)*abb", 4), (r"(ab|ac)", 3), (r"a{2}|b{1,}", 4),
                            (r"(yes|no|maybe)", 9), (r"(a|b)*a(a|b){3}", 16), (r"(aa)*|(aaa)*", 6), (r"é", 3),
                            (r".", 9), (r"x{0,40}", 41)):
        assert compile_dfa("regex", pattern)[0].shape[0] == states, pattern
    for a, b in ((r"(ab|ac)", r"a[bc]"), (r"(abc|bca)+", r"(?:bca|abc){1,}"), (r"a{2,3}", r"aaa?"),
                 (r"(a|b)*abb", r"(b|a)*abb"), (r"\d+", r"[0-9][0-9]*"), (r"(a*)*b", r"a*b")):
        (ta, fa), (tb, fb) = compile_dfa("regex", a), compile_dfa("regex", b)
        assert np.array_equal(ta, tb) and np.array_equal(fa, fb), (a, b)
    (ta, fa), (tb, fb) = compile_dfa("choice", ["ab", "ac"]), compile_dfa("regex", "a(b|c)")
    assert np.array_equal(ta, tb) and np.array_equal(fa, fb)


def test_compile_work_is_bounded_by_the_caps():
    """The heaviest patterns the caps admit, and ones just past them, at the default 1024 token-level states and
    32000 tokens: each compiles or is refused within 10 s (about 2 s where this was written; the bound leaves
    room for a slower machine). Before the caps bounded the work such patterns ran for minutes."""
    import time
    tb, eos = synthetic_vocab(32000)
    assert guided.dfa_limit(1024) == 4352 and guided.dfa_limit(10 ** 6) == guided.MAX_DFA_STATES
    for pattern, outcome in ((r"a{256}", 257), (r"((a|b)?){256}c", 258), (r"(a{32}){32}", "max_states = 1024"),
                             (r"(.?){200}", "max_states = 1024"), (r"(a|b)*a(a|b){14}", "4352 byte-level states"),
                             (r"((a{256}){256}){256}", "too large"), (r"(a{64}){64}", "too large")):
        t0 = time.perf_counter()
        if isinstance(outcome, int):
            assert compile_guide("regex", pattern, tb, eos, 1024).n_states == outcome
        else:
            with pytest.raises(SamplingError, match=outcome):
                compile_guide("regex", pattern, tb, eos, 1024)
        assert time.perf_counter() - t0 < 10.0, pattern


def test_accepted_strings_are_valid_utf8():
    trans, accept = compile_dfa("regex", r".[^a]\W")
    for raw in (b"\xc3", b"\xc3\x28", b"\xe2\x82", b"\xed\xa0\x80", b"\xc0\x80", b"\xf4\x90\x80\x80", b"\x80"):
        s = 0
        for b in raw:
            s = trans[s, b] if s >= 0 else -1
        assert s < 0 or not accept[s]
        if len(raw) > 1 or raw == b"\x80":
            assert not any(_accepts(trans, accept, raw + tail) for tail in (b"", b"!!", b"!"))
    assert _accepts(trans, accept, "é日!".encode()) and _accepts(trans, accept, "\U0001F680b ".encode())


def _accepts(trans, accept, data):
    s = 0
    for b in data:
        s = trans[s, b]
        if s < 0:
            return False
    return bool(accept[s])


def test_choice_is_the_alternation_of_the_escaped_strings():
    g = compile_guide("choice", ["a.b", "(x)", "a.b", "日本"], *synthetic_vocab())
    for s, ok in (("a.b", True), ("(x)", True), ("日本", True), ("axb", False), ("x", False), ("", False), ("a.b(x)", False)):
        assert g.matches(s.encode()) == ok, s
    assert g.viable(b"a.") and g.viable("日".encode()) and not g.viable(b"b")


ENGINE_PATTERNS = [r"(yes|no|maybe)", r"[0-9]{3}-[0-9]{4}", r"-?[1-9][0-9]*(\.[0-9]+)?"]


def _bytelevel_tokenizer(tmp_path):
    from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer
    from tests.test_checkpoint import _tokenizer_dir
    _tokenizer_dir(str(tmp_path))
    return Tokenizer(str(tmp_path))


def test_token_bytes_of_a_bytelevel_tokenizer(tmp_path):
    tok = _bytelevel_tokenizer(tmp_path)
    tb = tok.token_bytes()
    n = tok.tok.get_vocab_size()  # the trainer asks for 400 and stops when the text has no more merges
    assert len(tb) == n > 300 and tok.token_bytes() is tb
    assert sorted(t for t in tb if len(t) == 1) == [bytes([b]) for b in range(256)]  # the whole alphabet, inverted
    special = {tok.tok.token_to_id("<s>"), tok.tok.token_to_id("</s>")}
    assert all((tb[i] == b"") == (i in special) for i in range(n))
    text = "ünïcödé text and emoji 🚀 should round-trip, hello world"
    ids = tok.encode(text, special=False)
    assert b"".join(tb[i] for i in ids).decode() == text
    assert any(len(t) > 3 for t in tb)  # merges


def test_token_bytes_of_a_metaspace_vocabulary_and_of_an_unknown_kind(tmp_path):
    from tokenizers import Tokenizer as T, decoders, models, pre_tokenizers
    from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer
    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2, "<0x0A>": 3, "<0xC3>": 4, "▁the": 5, "▁": 6, "a": 7, "é": 8}
    raw = T(models.BPE(vocab=vocab, merges=[], unk_token="<unk>", byte_fallback=True))
    raw.pre_tokenizer = pre_tokenizers.Metaspace()
    raw.decoder = decoders.Metaspace()
    raw.add_special_tokens(["<unk>", "<s>", "</s>"])
    raw.save(str(tmp_path / "tokenizer.json"))
    tb = Tokenizer(str(tmp_path)).token_bytes()
    assert tb == [b"", b"", b"", b"\n", b"\xc3", b" the", b" ", b"a", "é".encode()]
    other = T(models.WordLevel(vocab={"a": 0, "[UNK]": 1}, unk_token="[UNK]"))
    (tmp_path / "w").mkdir()
    other.save(str(tmp_path / "w" / "tokenizer.json"))
    with pytest.raises(ValueError, match="ByteLevel BPE and Metaspace"):
        Tokenizer(str(tmp_path / "w")).token_bytes()


def _vocabularies(tmp_path):
    tok = _bytelevel_tokenizer(tmp_path)
    return [synthetic_vocab(), (tok.token_bytes(), sorted(tok.eos_ids))]


def test_token_table_against_a_brute_force_walk(tmp_path):
    for tb, eos in _vocabularies(tmp_path):
        for kind, pattern in [("regex", p) for p in ENGINE_PATTERNS] + \
                [("regex", r"(hello|world)( the)?\s\w{1,3}"), ("regex", r".{0,3}"), ("choice", ["hello world", "hell", "ünï"])]:
            g = compile_guide(kind, pattern, tb, eos, 256)
            want, accepting = brute_table(g, tb, eos)
            assert g.next.dtype == np.int16 and g.next.shape == want.shape == (g.n_states, len(tb))
            assert np.array_equal(g.next, want), (kind, pattern)
            assert np.array_equal(g.accepting, accepting)
            # EOS exactly in accepting states, and it leaves the state as it is
            for e in eos:
                assert np.array_equal(g.next[:, e], np.where(accepting, np.arange(g.n_states), -1))
            # tokens without bytes are never allowed
            empty = [t for t, b in enumerate(tb) if not b and t not in eos]
            assert empty and (g.next[:, empty] == -1).all()
            # every row is reachable from row 0 over token transitions, in breadth-first order
            seen = [0]
            for s in seen:
                for t in np.unique(g.next[s][g.next[s] >= 0]):
                    if int(t) not in seen:
                        seen.append(int(t))
            assert seen == list(range(g.n_states))


def test_states_no_token_sequence_reaches_get_no_row():
    tb, eos = synthetic_vocab()
    only = [t for t in range(len(tb)) if tb[t] in (b"abc", b"bca")]
    tb2 = [b if t in only or t in eos else b"" for t, b in enumerate(tb)]
    g = compile_guide("regex", r"(abc|bca)+", tb2, eos, 64)
    trans, _ = compile_dfa("regex", r"(abc|bca)+")
    assert trans.shape[0] > g.n_states == 2  # the byte DFA's inner states are gone: start, and "after a word"
    assert g.next[0, only].tolist() == [1, 1] and not g.accepting[0] and g.accepting[1]
    assert g.key != compile_guide("regex", r"(abc|bca)+", tb, eos, 64).key
    assert g.key == compile_guide("regex", r"(?:bca|abc){1,}", tb2, eos, 64).key  # the same table: one residency


REFUSED = [(r"(a)\1", "back-references"), (r"(?P<n>a)(?P=n)", "named groups"), (r"(?=a)b", "look-around"),
           (r"(?<!a)b", "look-around"), (r"a*?", "lazy"), (r"a{2,3}?", "lazy"), (r"a++", "possessive"),
           (r"(?i)a", "inline flags"), (r"^a", "anchors"), (r"a$", "anchors"), (r"\bfoo", r"\\b"),
           (r"\Afoo", r"\\A"), (r"a{300}", "counted repeats above 256"), (r"a{2,1}", "below its minimum"),
           (r"a{2}{3}", "multiple repeat"), (r"a**", "multiple repeat"), ("(" * 33 + "a" + ")" * 33, "deeper than 32"),
           (r"(a{64}){64}", "too large.*8387 automaton states, at most 4096"),
           (r"(a", r"missing '\)'"), (r"a)", "unbalanced"), (r"[a", r"missing '\]'"), (r"*a", "nothing to repeat"),
           (r"[é]", "non-ASCII characters in a class"), (r"\p{L}", r"escape \\p"), (r"a\x4", "two hex digits")]


def test_refusals_name_the_reason():
    tb, eos = synthetic_vocab()
    for pattern, reason in REFUSED:
        with pytest.raises(SamplingError, match=reason):
            compile_guide("regex", pattern, tb, eos, 64)
    with pytest.raises(SamplingError, match="at most 2048 characters"):
        compile_guide("regex", "a" * 2049, tb, eos, 64)
    with pytest.raises(SamplingError, match="at most 256 strings"):
        compile_guide("choice", [f"c{i}" for i in range(257)], tb, eos, 64)
    for bad in ([], ["a", ""], "ab", [1]):
        with pytest.raises(SamplingError, match="non-empty list of non-empty strings"):
            compile_guide("choice", bad, tb, eos, 64)
    with pytest.raises(SamplingError, match="at least one EOS"):
        compile_guide("regex", "a", tb, [], 64)
    with pytest.raises(SamplingError, match="inside the vocabulary"):
        compile_guide("regex", "a", tb, [len(tb)], 64)
    no_z = [b"" if b == b"z" else b for b in tb]  # a vocabulary that lacks a needed byte
    with pytest.raises(SamplingError, match="cannot be completed with this vocabulary"):
        compile_guide("regex", "az", no_z, eos, 64)
    with pytest.raises(SamplingError, match="more than max_states = 5"):
        compile_guide("regex", "[0-9]{3}-[0-9]{4}", tb, eos, 5)
    assert compile_guide("regex", "[0-9]{3}-[0-9]{4}", tb, eos, 9).n_states == 9
    with pytest.raises(SamplingError, match='"regex" or a "choice"'):
        compile_guide("json", "a", tb, eos, 64)


def test_emulation_over_several_steps_with_mixed_rows():
    """Three slots decode side by side: slot 0 guided by a phone number, slot 1
    not guided, slot 2 by a choice; the 'model' prefers tokens by a fixed random
    score. Greedy ids through the emulation spell full matches, the unguided row
    is a copy and keeps its id, and the states follow the host walk."""
    tb, eos = synthetic_vocab()
    V = len(tb)
    g0 = compile_guide("regex", ENGINE_PATTERNS[1], tb, eos, 64)
    g2 = compile_guide("choice", ["maybe", "no"], tb, eos, 64)
    arena = np.full((40, V), -1, dtype=np.int16)
    arena[3:3 + g0.n_states] = g0.next
    arena[20:20 + g2.n_states] = g2.next
    base, cur = np.array([3, -1, 20, 3], dtype=np.int32), np.zeros(4, dtype=np.int32)  # slot 3: guided, no rows
    cur[3] = 2
    rng = np.random.default_rng(0)
    slot, tok = np.array([0, 1, 2]), np.zeros(3, dtype=np.int64)
    outs = [[], [], []]
    for step in range(12):
        x = (np.float32(rng.standard_normal((3, V)) * 3).view(np.uint32) >> 16).astype(np.uint16)
        ids = np.array([guide_ref.bf16_argmax(r) for r in x])
        dec = np.full(3, int(step > 0))
        work, got, cur = guide_ref.guide(x, ids, tok, dec, slot, base, cur, arena)
        assert np.array_equal(work[1], x[1]) and got[1] == ids[1]
        for r, (g, b) in ((0, (g0, 3)), (2, (g2, 20))):
            allowed = arena[b + cur[r]] >= 0
            assert np.array_equal(work[r][allowed], x[r][allowed]) and (work[r][~allowed] == 0xFF80).all()
            assert allowed[got[r]]
        assert base.tolist() == [3, -1, 20, 3] and cur[3] == 2 and cur[1] == 0
        for r in range(3):
            outs[r].append(int(got[r]))
        tok = got
    for r, g in ((0, g0), (2, g2)):
        text, ended = completion(outs[r], tb, eos)
        assert ended and g.matches(text), (r, text)
        assert all(t in eos for t in outs[r][outs[r].index(next(t for t in outs[r] if t in eos)):])  # only EOS after it
    case = random_case(16, 1000, seed=3)
    work, ids, cur = case["want"]
    assert (work != case["x"]).any() and (ids != case["ids"]).any() and (cur != case["cur"]).any()


def test_request_parsing():
    assert guided_params({}) is None and guided_params({"guided_regex": None, "structured_outputs": None}) is None
    assert guided_params({"guided_regex": "a+"}) == ("regex", "a+")
    assert guided_params({"guided_choice": ["a", "b"]}) == ("choice", ("a", "b"))
    assert guided_params({"structured_outputs": {"regex": "a+"}}) == ("regex", "a+")
    assert guided_params({"structured_outputs": {"choice": ["x"], "regex": None}}) == ("choice", ("x",))
    for body, name in (({"guided_regex": 5}, "guided_regex must be a string"),
                       ({"guided_regex": ["a"]}, "guided_regex must be a string"),
                       ({"guided_choice": "ab"}, "guided_choice must be a non-empty list"),
                       ({"guided_choice": []}, "guided_choice must be a non-empty list"),
                       ({"guided_choice": ["a", ""]}, "guided_choice must be a non-empty list"),
                       ({"guided_choice": ["a", 1]}, "guided_choice must be a non-empty list"),
                       ({"structured_outputs": "a"}, "structured_outputs must be an object"),
                       ({"structured_outputs": {"json": {}}}, "structured_outputs.json is not supported"),
                       ({"structured_outputs": {"regex": 1}}, "structured_outputs.regex must be a string"),
                       ({"structured_outputs": {"choice": "a"}}, "structured_outputs.choice must be a non-empty"),
                       ({"guided_regex": "a", "guided_choice": ["a"]}, "guided_regex and guided_choice cannot"),
                       ({"guided_regex": "a", "structured_outputs": {"regex": "a"}}, "cannot be combined"),
                       ({"structured_outputs": {"regex": "a", "choice": ["a"]}}, "cannot be combined")):
        with pytest.raises(SamplingError, match=name):
            guided_params(body)
    # The keys take no part in sampling_params: with or without the switch they are not "unsupported parameters".
    s = sampling_params({"guided_regex": "a", "guided_choice": ["x"], "structured_outputs": {"regex": 1}}, False)
    assert s.greedy


class _FakeModel:
    """next = (31 * token + pos + 7) % vocab (as in test_inference_server)."""

    def __init__(self, vocab, max_seq=256):
        self.cfg = SimpleNamespace(vocab=vocab, max_seq=max_seq)
        self.device = torch.device("cpu")
        self.scratch_slot = 4

    def decode_step(self, tokens, pos, pos_range, slots=None):
        return (tokens * 31 + pos.to(torch.int64) + 7) % self.cfg.vocab


def _collect(req):
    out = []
    while (t := req.out.get(timeout=20)) is not None:
        out.append(t)
    return out


def test_eager_engine_refuses_guides_and_a_server_without_the_switch_ignores_the_keys(tmp_path):
    import http.client
    from p2p_llm_tunnel_amd.models.server import start_server
    tb, eos = synthetic_vocab()
    g = compile_guide("regex", "a+", tb, eos, 16)
    with pytest.raises(ValueError, match="guided decoding needs the graph-captured HIP step"):
        Engine(max_batch=4, model=_FakeModel(len(tb)), guided=True)
    with pytest.raises(TypeError, match="guided.Guide"):
        Request([1], 2, guide="a+")
    with pytest.raises(ValueError, match="takes no guide"):
        Request([1], 2, embed="mean", guide=g)
    eng = Engine(max_batch=4, model=_FakeModel(len(tb)))
    try:
        assert not eng.guided
        with pytest.raises(ValueError, match="guided=True"):
            eng.submit(Request([1, 2], 3, guide=g))
        plain = _collect(eng.submit(Request([1, 2], 3)))
        with pytest.raises(ValueError, match="built without it"):
            start_server(port=0, engine=eng, guided=True)
        srv, port, _ = start_server(port=0, engine=eng, model_name="fake")
        try:
            c = http.client.HTTPConnection("127.0.0.1", port, timeout=20)
            texts = []
            for extra in ({}, {"guided_regex": "(a", "guided_choice": 7, "structured_outputs": "x"}):
                c.request("POST", "/v1/completions", body=json.dumps({"prompt": "\x01\x02", "max_tokens": 3, **extra}))
                r = c.getresponse()
                assert r.status == 200
                texts.append(json.loads(r.read())["choices"][0]["text"])
            assert texts[0] == texts[1] == "".join(f" t{t}" for t in plain)
        finally:
            srv.shutdown()
    finally:
        eng.stop()


def test_switches_reach_the_replicas():
    from p2p_llm_tunnel_amd.models.server import arg_parser, replica_cmd
    a = arg_parser().parse_args(["--gpus", "2", "--guided", "--guided-states", "300"])
    assert replica_cmd(a, 1)[-3:] == ["--guided", "--guided-states", "300"]
    assert "--guided" not in replica_cmd(arg_parser().parse_args(["--gpus", "2"]), 0)
    assert guided.MAX_REPEAT == 256 and guided.MAX_PATTERN == 2048 and guided.MAX_CHOICES == 256
