"""Evaluation rule of the reference (src/train.py:260-272, src/test.py:61-74): accuracy and weighted-F1 are computed
PER BATCH with scikit-learn on the valid (label != -1) utterances, then averaged UNWEIGHTED over the batches."""
import torch
from sklearn.metrics import accuracy_score, f1_score


def move_batch(batch, device, non_blocking=False, text_encoder=None, audio_encoder=None):
    """The four tensors of a collated batch on `device`: text, audio, emotion, padding_mask.
    text_encoder (a ``mer_amd.roberta.RobertaEncoder``; `runtime.text_encoder`, BASELINE config C5): the batch carries token ids
    ("text_ids" / "text_mask", [B, L, S]) and the text rows are computed HERE - the [CLS] hidden state of every valid utterance
    (src/feature_extractors/text/embeddings.py:83 of the reference, which dumps those rows to disk in a separate stage), under
    inference_mode (the reference fine-tunes the encoder in its own stage; the fusion model trains on its outputs), pads zero.
    audio_encoder (a ``mer_amd.wav2vec2.Wav2Vec2Encoder``; `runtime.audio_encoder`): the batch carries the waveforms of its utterances
    ("waveforms" / "wave_lengths" / "wave_index") and the audio rows are computed HERE, all utterances of the batch in one encoder
    batch - the mean of each one's valid wav2vec2 frames (src/feature_extractors/audio_wav2vec2/embeddings.py:77-85), pads zero."""
    emotion, mask = (batch[k].to(device, non_blocking=non_blocking) for k in ("emotion", "padding_mask"))
    if audio_encoder is not None and "waveforms" in batch:
        B, L = mask.shape
        wav = batch["waveforms"].to(device, non_blocking=non_blocking)
        lens = batch["wave_lengths"].to(device, non_blocking=non_blocking)
        idx = batch["wave_index"].to(device, non_blocking=non_blocking)
        with torch.inference_mode():
            rows = audio_encoder.utterance_embeddings(wav, lens).float()
        audio = torch.zeros(B * L, rows.shape[1], dtype=torch.float32, device=device)
        audio[idx] = rows.clone()
        audio = audio.view(B, L, -1)
    else:
        audio = batch["audio"].to(device, non_blocking=non_blocking)
    if text_encoder is None or "text_ids" not in batch:
        return batch["text"].to(device, non_blocking=non_blocking), audio, emotion, mask
    ids, am = batch["text_ids"].to(device, non_blocking=non_blocking), batch["text_mask"].to(device, non_blocking=non_blocking)
    B, L, S = ids.shape
    valid = ~mask
    with torch.inference_mode():
        cls = text_encoder.cls_embeddings(ids[valid].contiguous(), am[valid].contiguous()).float()
    text = torch.zeros(B, L, cls.shape[1], dtype=torch.float32, device=device)
    text[valid] = cls.clone()
    return text, audio, emotion, mask


class BatchScores:
    def __init__(self):
        self.n_batches = 0
        self._acc = 0.0
        self._f1 = 0.0

    def update(self, logits: torch.Tensor, emotion: torch.Tensor) -> None:
        valid = emotion != -1
        predicted = logits.argmax(dim=2)[valid].reshape(-1).cpu().numpy()
        target = emotion[valid].reshape(-1).cpu().numpy()
        self._acc += accuracy_score(target, predicted)
        self._f1 += f1_score(target, predicted, average="weighted")
        self.n_batches += 1

    def sums(self):
        """(sum of per-batch accuracies, sum of per-batch weighted-F1s) - what ranks add up under data parallelism."""
        return self._acc, self._f1

    def result(self):
        """(accuracy, weighted_f1), each the plain mean of the per-batch scores."""
        n = max(self.n_batches, 1)
        return self._acc / n, self._f1 / n
