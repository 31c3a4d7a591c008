"""BERTScore (Zhang et al. 2020) on the project's own encoder and kernels: what the reference's evaluation half calls as
`bert_score.score(preds, refs, lang='vi', model_type=args.bert_score_model, num_layers=12)` (run_pretraining_fcmf.py:434,575).

The `bert_score` package is a sentence encoder plus a greedy cosine matching.  The encoder is `roberta.RobertaModel` (the HIP
RoBERTa that an HF directory such as uitnlp/visobert loads into), stopped after `num_layers` layers as the package truncates its
model; the matching is `ops.bertscore` (csrc/bertscore.hip).  Token weights are 1, and 0 on the first and last token of a
sentence (<s>, </s>), which still serve as match targets of the other side; a sentence of only those two scores 0.
NOT built: idf weighting, baseline rescaling (the reference's call uses neither), ROUGE.  The package is not importable offline,
so the definition in include/fcmf_hip.h is the contract rather than parity with the package.
"""
import torch

from . import ops
from .roberta import RobertaModel

__all__ = ["BertScorer", "score"]

MAX_TOKENS = 512      # fcmf_bertscore's limit, the encoder's position limit


class BertScorer:
    def __init__(self, model, num_layers=12, batch_size=64, device=None):
        """model: a local HF model directory (RobertaModel.from_pretrained refuses anything else) or a RobertaModel;
        num_layers is clamped to the model's depth; batch_size sentences per encoder call"""
        if not isinstance(model, RobertaModel):
            model = RobertaModel.from_pretrained(model)
            model = model.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
        elif device is not None:
            model = model.to(device)
        self.model = model.eval()
        cfg = model.config
        self.num_layers = max(1, min(int(num_layers), cfg.num_hidden_layers))
        self.batch_size = int(batch_size)
        self.pad_id = cfg.pad_token_id
        # RoBERTa positions start at pad_id + 1
        self.max_tokens = min(MAX_TOKENS, cfg.max_position_embeddings - cfg.pad_token_id - 1)

    @property
    def device(self):
        return self.model.embeddings.word_embeddings.weight.device

    @torch.no_grad()
    def embed(self, sentences):
        """token-id lists -> ([n, L_max, H] layer-`num_layers` embeddings in the compute dtype, lengths int32 [n], both on the
        device, in input order).  Sentences are encoded sorted by length, `batch_size` at a time, padded with pad_token_id under an
        attention mask built from the lengths; rows beyond a sentence's length hold whatever the encoder made of the padding."""
        n = len(sentences)
        lens = [len(s) for s in sentences]
        if n and (min(lens) < 1 or max(lens) > self.max_tokens):
            raise ValueError(f"BertScorer: sentences must hold 1..{self.max_tokens} token ids (got {min(lens)}..{max(lens)})")
        V = self.model.config.vocab_size
        if any(not 0 <= int(t) < V for s in sentences for t in s):           # (the embedding gather does not check its indices)
            raise ValueError(f"BertScorer: token id outside the scorer model's vocabulary of {V}")
        dev = self.device
        was_training = self.model.training
        self.model.eval()
        Lmax = max(lens, default=1)
        out = None
        order = sorted(range(n), key=lambda i: lens[i])
        for b in range(0, n, self.batch_size):
            idx = order[b:b + self.batch_size]
            S = lens[idx[-1]]
            ids = torch.full((len(idx), S), self.pad_id, dtype=torch.long)
            for r, i in enumerate(idx):
                ids[r, :lens[i]] = torch.as_tensor(sentences[i], dtype=torch.long)
            blen = torch.tensor([lens[i] for i in idx])
            mask = (torch.arange(S)[None, :] < blen[:, None]).long()
            seq = self.model.encode(ids.to(dev), None, mask.to(dev), num_layers=self.num_layers)
            if out is None:
                out = torch.zeros((n, Lmax, seq.shape[-1]), dtype=seq.dtype, device=dev)
            out[torch.tensor(idx, device=dev), :S] = seq
        if out is None:
            out = torch.zeros((0, 1, self.model.config.hidden_size), dtype=ops.compute_dtype(), device=dev)
        self.model.train(was_training)
        return out, torch.tensor(lens, dtype=torch.int32, device=dev)

    @staticmethod
    def _weights(lens, L, dev):
        w = (torch.arange(L)[None, :] < lens[:, None]).float()
        rows = torch.arange(len(lens))
        w[rows, 0] = 0.0
        w[rows, (lens - 1).clamp(min=0).long()] = 0.0
        return w.to(dev)

    @torch.no_grad()
    def score_ids(self, cand_ids, ref_ids):
        """two equal-length lists of token-id lists, each with its <s> ... </s> -> (P, R, F) float32 [n], in input order"""
        if len(cand_ids) != len(ref_ids):
            raise ValueError(f"BertScorer: {len(cand_ids)} candidates against {len(ref_ids)} references")
        n = len(cand_ids)
        if n == 0:
            z = torch.zeros(0, dtype=torch.float32, device=self.device)
            return z, z.clone(), z.clone()
        cand, clen = self.embed(cand_ids)
        ref, rlen = self.embed(ref_ids)
        out = ops.bertscore(cand, ref, clen, rlen, self._weights(clen.cpu(), cand.shape[1], cand.device),
                            self._weights(rlen.cpu(), ref.shape[1], ref.device))
        return out[:, 0].contiguous(), out[:, 1].contiguous(), out[:, 2].contiguous()

    def tokenize(self, texts, tokenizer):
        out = []
        for t in texts:
            ids = list(tokenizer.encode(str(t).strip(), add_special_tokens=True, truncation=True, max_length=self.max_tokens))
            if len(ids) < 2:                                     # an empty string is <s> </s>
                first = tokenizer.cls_token_id if tokenizer.cls_token_id is not None else tokenizer.bos_token_id
                ids = [first, tokenizer.sep_token_id]
            out.append(ids)
        return out

    def score(self, cands, refs, tokenizer):
        """texts -> (P, R, F): `text.strip()` encoded with its special tokens, truncated to the model's positions"""
        return self.score_ids(self.tokenize(cands, tokenizer), self.tokenize(refs, tokenizer))


_scorers = {}


def score(cands, refs, lang=None, model_type=None, num_layers=12, device=None, verbose=False, tokenizer=None):
    """the call of the reference's evaluation half: -> (P, R, F1), float32 [n] each.  model_type must be a LOCAL model directory
    (nothing is fetched); `lang` and `verbose` are accepted and unused; tokenizer: default the one stored in that directory."""
    if model_type is None:
        raise ValueError("score: model_type (a local model directory) is required")
    key = (str(model_type), int(num_layers), str(device))
    if key not in _scorers:
        _scorers[key] = BertScorer(model_type, num_layers=num_layers, device=device)
    if tokenizer is None:
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(model_type, local_files_only=True)
    return _scorers[key].score(cands, refs, tokenizer)
