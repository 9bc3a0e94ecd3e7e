"""Dialogue-level dataset with the reference's surface (``src/dataset.py``): ``Dataset(mode)``, ``__getitem__``
-> {"text": [n, d_t], "audio": [n, d_a], "emotion": list of [1] tensors}, ``collate_fn`` -> {"text": [B, L, d_t],
"audio": [B, L, d_a], "padding_mask": bool [B, L], "emotion": int64 [B, L] (-1 on pads)}.

Unlike the reference (three full-DataFrame scans per utterance, src/dataset.py:35,43-45) the dialogue -> row
index is built ONCE at construction, so ``__getitem__`` is two tensor gathers."""
import os
import pickle
import wave

import numpy as np
import torch

from utils import get_config, get_text

EMOTIONS = {"neutral": 0, "joy": 1, "sadness": 2, "anger": 3, "surprise": 4, "fear": 5, "disgust": 6}
SENTIMENTS = {"neutral": 0, "positive": 1, "negative": 2}          # MELD's second label per utterance (runtime.aux_head)


def build_dialogue_index(dialogue_ids, utterance_ids):
    """Rows of each dialogue in Utterance_ID order; dialogues in order of first appearance."""
    dialogue_ids = np.asarray(dialogue_ids)
    utterance_ids = np.asarray(utterance_ids)
    order = {}
    for row, d in enumerate(dialogue_ids.tolist()):
        order.setdefault(d, []).append(row)
    index = []
    for d, rows in order.items():
        rows = np.asarray(rows)
        index.append(rows[np.argsort(utterance_ids[rows], kind="stable")])
    return list(order.keys()), index


def tokenised_contexts(table, tokenizer, max_tokens=64):
    """Token ids of every utterance WITH ITS CONTEXT, the input of the in-loop text encoder (BASELINE C5; `runtime.text_encoder`):
    the strings of the reference's text feature extractor (src/feature_extractors/text/dataset.py:28-34 -> utils.py:61-92,
    restated in mer_amd.text_context), tokenised by the CALLER's tokenizer the way that dataset does (:36-44: padding to
    max_length, truncation) -> (int64 ids [N, max_tokens], int64 mask [N, max_tokens]) in table row order."""
    from mer_amd.text_context import build_contexts
    texts = build_contexts(table["Utterance"].tolist(), table["Dialogue_ID"].tolist(), table["Utterance_ID"].tolist(), tokenizer.sep_token)
    enc = tokenizer(texts, padding="max_length", truncation=True, max_length=int(max_tokens), return_tensors="pt")
    return enc["input_ids"].to(torch.int64), enc["attention_mask"].to(torch.int64)


WAV_SAMPLE_RATE = 16000
WAV_MAX_SECONDS = 10


def load_wav(path, max_seconds=WAV_MAX_SECONDS):
    """One utterance's waveform as the reference's wav2vec2 stage reads it (src/feature_extractors/audio_wav2vec2/dataset.py:37-48):
    mono, 16 kHz, float in [-1, 1) (16-bit PCM / 32768), truncated to 10 s.  The files are what the reference's scripts/mp4towav.py
    writes (ffmpeg -ac 1 -ar 16000); there is no resampler here, so other rates, channel counts and sample widths are refused."""
    with wave.open(os.fspath(path), "rb") as w:
        if w.getframerate() != WAV_SAMPLE_RATE:
            raise ValueError(f"{path}: {w.getframerate()} Hz; only {WAV_SAMPLE_RATE} Hz is read (there is no resampler)")
        if w.getnchannels() != 1 or w.getsampwidth() != 2 or w.getcomptype() != "NONE":
            raise ValueError(f"{path}: need mono 16-bit PCM (got {w.getnchannels()} channel(s), {8 * w.getsampwidth()}-bit, {w.getcomptype()})")
        n = min(w.getnframes(), int(max_seconds * WAV_SAMPLE_RATE))
        pcm = np.frombuffer(w.readframes(n), dtype="<i2")
    return torch.from_numpy(pcm.astype(np.float32) / 32768.0)


def load_waveforms(table, wav_dir, max_seconds=WAV_MAX_SECONDS):
    """Waveforms of every table row, in row order: wav_dir/dia{Dialogue_ID}_utt{Utterance_ID}.wav (the reference's file names)."""
    return [load_wav(os.path.join(os.fspath(wav_dir), f"dia{d}_utt{u}.wav"), max_seconds)
            for d, u in zip(table["Dialogue_ID"].tolist(), table["Utterance_ID"].tolist())]


def dialogue_speaker_ids(speakers, rows):
    """Per-dialogue speaker ids: the `Speaker` column's values of every table row -> int64 [N], the speakers of a dialogue numbered
    0, 1, 2, ... in order of first appearance inside it (`rows`: the dialogues' row indices in utterance order, `build_dialogue_index`).
    Only equality inside a dialogue matters to the model; more than 256 speakers in one dialogue are refused (ids are one byte)."""
    speakers = list(speakers)
    out = np.zeros(len(speakers), dtype=np.int64)
    for d, idx in enumerate(rows):
        seen = {}
        for r in np.asarray(idx).tolist():
            out[r] = seen.setdefault(speakers[r], len(seen))
        if len(seen) > 256:
            raise ValueError(f"dialogue {d} has {len(seen)} speakers; speaker ids are one byte (at most 256 per dialogue)")
    return torch.as_tensor(out)


class Dataset(torch.utils.data.Dataset):
    def __init__(self, mode="train", text_embeddings=None, audio_embeddings=None, table=None, token_ids=None, token_mask=None,
                 waveforms=None, speakers=False, sentiment=False):
        """sentiment (runtime.aux_head is enabled): items ALSO carry "sentiment" - int64 [n], `SENTIMENTS` of the table's `Sentiment`
        column, anything else -1 - and batches "sentiment" int64 [B, L], padded with -1 like the emotion.
        speakers (runtime.speaker_heads is set): items ALSO carry "speaker" - int64 [n], `dialogue_speaker_ids` of the table's
        `Speaker` column - and batches "speaker" int64 [B, L], padded with 0 (M2FNet(speaker_heads=...) reads them; pad slots are ignored).
        token_ids / token_mask ([N, S] int64, rows = table rows; `tokenised_contexts`): items and batches ALSO carry "text_ids" /
        "text_mask" - what the in-loop text encoder consumes instead of the pre-extracted "text" rows (`runtime.text_encoder`).
        waveforms (a list of 1-D float tensors, rows = table rows; `load_waveforms`): items carry "wave" and batches "waveforms" /
        "wave_lengths" / "wave_index" - what the in-loop audio encoder consumes (`runtime.audio_encoder`); the audio pickle is then
        not read (audio_embeddings stays optional)."""
        super().__init__()
        self.mode = mode
        self.token_ids, self.token_mask = token_ids, token_mask
        self.waveforms = waveforms
        if waveforms is not None:
            if text_embeddings is None:
                with open(os.path.join(os.path.abspath(get_config().embeddings.text), f"{mode}.pkl"), "rb") as f:
                    text_embeddings = pickle.load(f)
        elif text_embeddings is None or audio_embeddings is None:
            config = get_config()
            with open(os.path.join(os.path.abspath(config.embeddings.text), f"{mode}.pkl"), "rb") as f:
                text_embeddings = pickle.load(f)
            with open(os.path.join(os.path.abspath(config.embeddings.audio), f"{mode}.pkl"), "rb") as f:
                audio_embeddings = pickle.load(f)
        self.text_embeddings, self.audio_embeddings = text_embeddings, audio_embeddings
        self.text = get_text(mode) if table is None else table
        self.text["Emotion"] = self.text["Emotion"].map(lambda e: EMOTIONS.get(e, e))
        self.dialogue_ids, self.rows = build_dialogue_index(self.text["Dialogue_ID"].to_numpy(),
                                                            self.text["Utterance_ID"].to_numpy())
        self._labels = torch.as_tensor(self.text["Emotion"].to_numpy().astype(np.int64))
        self._sentiment = None
        if sentiment:
            if "Sentiment" not in self.text:
                raise ValueError(f"runtime.aux_head needs the Sentiment column of the {mode} table")
            self._sentiment = torch.as_tensor(np.asarray([SENTIMENTS.get(v, -1) for v in self.text["Sentiment"].tolist()], dtype=np.int64))
        self._speakers = None
        if speakers:
            if "Speaker" not in self.text:
                raise ValueError(f"runtime.speaker_heads needs the Speaker column of the {mode} table")
            self._speakers = dialogue_speaker_ids(self.text["Speaker"].tolist(), self.rows)
        print(f"Loaded {len(self.dialogue_ids)} dialogues for {self.mode}ing")

    def __len__(self):
        return len(self.dialogue_ids)

    def __getitem__(self, idx):
        rows = torch.as_tensor(self.rows[idx])
        item = {"text": self.text_embeddings[rows], "emotion": [e.reshape(1) for e in self._labels[rows]]}
        if self.audio_embeddings is not None:
            item["audio"] = self.audio_embeddings[rows]
        if self.waveforms is not None:
            item["wave"] = [self.waveforms[r] for r in rows.tolist()]
        if self._speakers is not None:
            item["speaker"] = self._speakers[rows]
        if self._sentiment is not None:
            item["sentiment"] = self._sentiment[rows]
        if self.token_ids is not None:
            item["text_ids"] = self.token_ids[rows]
            item["text_mask"] = self.token_mask[rows] if self.token_mask is not None else torch.ones_like(item["text_ids"])
        return item

    def get_labels(self):
        return self.text["Emotion"].to_numpy()

    def get_dialogue_labels(self):
        """(labels, lengths): every dialogue's labels in utterance order, one dialogue after the other, and the utterances per dialogue
        - what `LinearChainCRF.from_label_counts` counts (runtime.crf.init: bigram)."""
        labels = self._labels.numpy()
        return np.concatenate([labels[np.asarray(r)] for r in self.rows]), np.asarray([len(r) for r in self.rows])


def collate_fn(batch):
    B = len(batch)
    L = max(d["text"].shape[0] for d in batch)
    text = batch[0]["text"].new_zeros(B, L, batch[0]["text"].shape[1])
    has_audio = "audio" in batch[0]
    audio = batch[0]["audio"].new_zeros(B, L, batch[0]["audio"].shape[1]) if has_audio else None
    emotion = torch.full((B, L), -1, dtype=torch.int64)          # -1 = ignored by the criterion
    for i, d in enumerate(batch):
        n = d["text"].shape[0]
        text[i, :n] = d["text"]
        if has_audio:
            audio[i, :n] = d["audio"]
        emotion[i, :n] = torch.cat([torch.as_tensor(e).reshape(1) for e in d["emotion"]]).to(torch.int64)
    out = {"text": text}
    if has_audio:
        out["audio"] = audio
    out["padding_mask"], out["emotion"] = emotion == -1, emotion
    if "speaker" in batch[0]:                                      # speaker heads: per-dialogue ids, 0 on pads (ignored there)
        speaker = torch.zeros(B, L, dtype=torch.int64)
        for i, d in enumerate(batch):
            speaker[i, : d["speaker"].shape[0]] = d["speaker"]
        out["speaker"] = speaker
    if "sentiment" in batch[0]:                                    # the auxiliary head's labels: -1 on pads, as the emotion
        sentiment = torch.full((B, L), -1, dtype=torch.int64)
        for i, d in enumerate(batch):
            sentiment[i, : d["sentiment"].shape[0]] = d["sentiment"]
        out["sentiment"] = sentiment
    if "wave" in batch[0]:
        # in-loop audio encoder: the waveforms of all utterances of the batch, zero-padded to the longest ([n, N] fp32), their sample
        # counts, and where each goes in the [B, L] grid (flat index b * L + t)
        waves = [w for d in batch for w in d["wave"]]
        lengths = torch.tensor([w.shape[0] for w in waves], dtype=torch.int64)
        wav = torch.zeros(len(waves), int(lengths.max()) if len(waves) else 0, dtype=torch.float32)
        for j, w in enumerate(waves):
            wav[j, : w.shape[0]] = w
        out["waveforms"], out["wave_lengths"] = wav, lengths
        out["wave_index"] = torch.cat([i * L + torch.arange(len(d["wave"]), dtype=torch.int64) for i, d in enumerate(batch)])
    if "text_ids" in batch[0]:                                     # in-loop text encoder: [B, L, S] token ids + attention mask, zero on pads
        S = batch[0]["text_ids"].shape[1]
        ids = torch.zeros(B, L, S, dtype=torch.int64)
        msk = torch.zeros(B, L, S, dtype=torch.int64)
        for i, d in enumerate(batch):
            n = d["text_ids"].shape[0]
            ids[i, :n], msk[i, :n] = d["text_ids"], d["text_mask"]
        out["text_ids"], out["text_mask"] = ids, msk
    return out


class DeviceLoader:
    """Drop-in for ``torch.utils.data.DataLoader(Dataset, collate_fn=collate_fn, batch_size, shuffle)`` with both embedding
    tables resident in HBM (``runtime.device_batcher: True``): one gather kernel per batch fills the same
    {"text", "audio", "padding_mask", "emotion"} dict, on the device, with dialogues in DataLoader order (a fresh
    ``torch.randperm`` per epoch when shuffling, the last batch partial - torch's ``drop_last=False`` default)."""

    def __init__(self, dataset, batch_size=32, shuffle=False, device="cuda", seed=None, **_ignored_loader_kwargs):
        from mer_amd.batcher import DeviceDialogueBatcher
        self.batch_size, self.shuffle = int(batch_size), bool(shuffle)
        self.n = len(dataset)
        self.batcher = DeviceDialogueBatcher(dataset.text_embeddings, dataset.audio_embeddings, dataset._labels, dataset.rows,
                                             device=device)
        self.generator = torch.Generator()
        if seed is not None:
            self.generator.manual_seed(int(seed))

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        order = torch.randperm(self.n, generator=self.generator).tolist() if self.shuffle else list(range(self.n))
        for start in range(0, self.n, self.batch_size):
            yield self.batcher.gather(order[start: start + self.batch_size])
