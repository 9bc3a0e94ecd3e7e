"""Drop-in for the reference's ``src/test.py``: load ``checkpoint.load_path`` and report accuracy / weighted-F1
on the test split (mean of per-batch sklearn scores, reference src/test.py:51-74)."""
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from dataset import Dataset, DeviceLoader, collate_fn  # noqa: E402
from metrics import BatchScores, move_batch  # noqa: E402
from model import M2FNet  # noqa: E402
from utils import get_config  # noqa: E402

try:
    from tqdm import tqdm
except ImportError:
    def tqdm(it, **_):
        return it


def load_model_weights(model, checkpoint_path, device, averaged: bool = False):
    """Checkpoint format of the training loop: {'epoch', 'model_state_dict', 'optimizer_state_dict'} and, from a run with
    runtime.ema enabled, 'ema_state_dict'.  averaged (runtime.ema.enabled and evaluate): the averaged weights are loaded when the
    checkpoint holds them.  Prints which weights were loaded."""
    checkpoint_path = os.path.abspath(checkpoint_path)
    if not os.path.exists(checkpoint_path):
        raise ValueError("Checkpoint not found")
    state = torch.load(checkpoint_path, map_location=device)
    if averaged and "ema_state_dict" in state:
        ema = state["ema_state_dict"]
        model.load_state_dict(ema["parameters"])
        print(f"Scoring the averaged weights (EMA, decay {ema['decay']}, {ema['n_averaged']} updates)")
    else:
        model.load_state_dict(state["model_state_dict"])
        print("Scoring the live weights (model_state_dict)")
    crf = getattr(model, "crf", None)                       # (solver.loss_fn: CRF; set by main())
    if crf is not None:
        if "crf_state_dict" not in state:
            raise ValueError("solver.loss_fn is CRF but the checkpoint holds no 'crf_state_dict'")
        crf.load_state_dict(state["crf_state_dict"])
        print("Decoding with the checkpoint's CRF (crf_state_dict)")
    head = getattr(model, "aux_head", None)                 # (runtime.aux_head; set by main())
    if head is not None:
        if "aux_head_state_dict" in state:
            head.load_state_dict(state["aux_head_state_dict"])
            print("Reporting the accuracy of the checkpoint's auxiliary head (aux_head_state_dict)")
        else:
            print("The checkpoint holds no 'aux_head_state_dict': the auxiliary accuracy is that of an untrained head")
    return state.get("epoch")


def streaming_settings(config):
    """`runtime.streaming`: True = test() scores every batch through a `DialogueStream` (M2FNet.stream) - each utterance labelled when it
    arrives, from the K / V caches of the utterances before it - instead of `forward`.  Needs a causal `runtime.context` (future: 0): a
    band that looks ahead cannot stream.  -> bool; checked on the host before the GPU is touched."""
    from train import _runtime, context_settings
    if not bool(_runtime(config, "streaming", False)):
        return False
    band = context_settings(config)
    if band is None or band[1] != 0:
        raise ValueError("runtime.streaming needs a causal runtime.context ({past: null or k, future: 0}): a band that looks ahead "
                         f"cannot label an utterance when it arrives (got {None if band is None else dict(past=band[0], future=band[1])})")
    return True


def stream_chunk_settings(config):
    """`runtime.stream_chunk`: 1 (default) = a streamed test pass feeds every batch column by column; T in 2 .. 64 = the stream is opened
    with `max_chunk=T` (M2FNet.stream) and `DialogueStream.run` feeds T columns per call through the chunk plan.  -> int; checked on the
    host before the GPU is touched."""
    from train import _runtime
    from mer_amd.streaming import resolve_max_chunk
    T = _runtime(config, "stream_chunk", 1)
    try:
        return resolve_max_chunk(1 if T is None else T)        # (the one statement of the range)
    except ValueError as e:
        raise ValueError(f"runtime.stream_chunk: {e}") from None


def stream_pages_settings(config):
    """`runtime.stream_pages`: 0 (default) = the streamed test pass keeps dense K / V caches; N >= 1 = the stream is opened with `pages=N`
    (M2FNet.stream: cache rows allocated in pages of 16 from a pool of N per site).  -> int; checked on the host before the GPU is
    touched."""
    from train import _runtime
    from mer_amd.streaming import resolve_pages
    N = _runtime(config, "stream_pages", 0)
    N = 0 if N is None else N
    if isinstance(N, bool) or not isinstance(N, int) or N < 0:
        raise ValueError(f"runtime.stream_pages: 0 (dense caches) or a number of pages >= 1, got {N!r}")
    try:
        return resolve_pages(N or None, 16)[0] or 0
    except ValueError as e:
        raise ValueError(f"runtime.stream_pages: {e}") from None


def attention_maps_settings(config):
    """`runtime.attention_maps`: {enabled, file, sites} - enabled: test() also writes the attention maps of the pass (M2FNet.last_attention:
    what need_weights=True returns, heads averaged) to `file`, one .npz with an array `<dialogue>/<site>` [n, n] per dialogue of the pass
    (in loader order, n its utterances) and site; sites: names of `mer_amd.layout.attention_sites` (empty or null: every site).  Not with
    runtime.streaming (a streamed pass has no [L, L] map; see DialogueStream.attention).  -> None or (file, sites or None); checked on
    the host before the GPU is touched."""
    from train import _runtime
    block = _runtime(config, "attention_maps", None)
    if not block or not block.get("enabled", False):
        return None
    if not isinstance(block.get("enabled"), bool):
        raise ValueError(f"runtime.attention_maps.enabled must be true or false, got {block.get('enabled')!r}")
    path = block.get("file", None)
    if not isinstance(path, str) or not path:
        raise ValueError(f"runtime.attention_maps.file must be the path of the .npz to write, got {path!r}")
    sites = block.get("sites", None)
    if sites is not None and (isinstance(sites, str) or not all(isinstance(n, str) for n in sites)):
        raise ValueError(f"runtime.attention_maps.sites must be a list of attention-site names, got {sites!r}")
    from mer_amd.layout import attention_sites
    names = [n for n, _, _ in attention_sites(config.model)]
    unknown = [n for n in (sites or []) if n not in names]
    if unknown:
        raise ValueError(f"runtime.attention_maps.sites: unknown attention site(s) {unknown}; this model has {names}")
    if bool(_runtime(config, "streaming", False)):
        raise ValueError("runtime.attention_maps does not combine with runtime.streaming: a streamed pass keeps no [L, L] maps "
                         "(DialogueStream.attention returns each step's rows)")
    return path, (list(sites) if sites else None)


class _MapCollector:
    """The maps of a test pass, per dialogue in loader order (`runtime.attention_maps`)."""

    def __init__(self, model):
        self.model, self.out = model, getattr(model, "attention_maps_out", None)
        self.arrays, self.n_dialogues = {}, 0

    def add(self, padding_mask) -> None:
        if self.out is None:
            return
        maps = {name: m.cpu().numpy() for name, m in self.model.last_attention(sites=self.out[1]).items()}
        for b, n in enumerate((~padding_mask.bool()).sum(1).tolist()):
            for name, m in maps.items():
                self.arrays[f"{self.n_dialogues}/{name}"] = m[b, :n, :n]
            self.n_dialogues += 1

    def write(self) -> None:
        if self.out is None:
            return
        import numpy as np
        with open(self.out[0], "wb") as f:                 # (an open file: numpy appends no suffix to the configured path)
            np.savez(f, **self.arrays)
        print(f"Wrote the attention maps of {self.n_dialogues} dialogues to {self.out[0]}")


def _stream_for(model, B, L):
    """The model's test stream, opened (again) when a batch has more dialogues or - without a window - longer ones than it holds."""
    st = getattr(model, "_test_stream", None)
    windowed = model.context[0] is not None
    chunk = getattr(model, "stream_chunk", 1)
    pages = getattr(model, "stream_pages", 0) or None
    if st is None or st.max_streams < B or (not windowed and st.capacity < L) or st.max_chunk != chunk or st.pages != pages:
        if st is not None:
            st.close()
        # (solver.loss_fn: CRF - the stream also runs the forward filter: stream.crf_posterior() is there for the caller; the pass
        #  below keeps the per-row argmax of the emission logits)
        st = model.stream(B, capacity=None if windowed else min(512, (L + 63) // 64 * 64), max_chunk=chunk, pages=pages,
                          crf=getattr(model, "crf", None))
        model._test_stream = st
    return st


def decoded(crf, logits, padding_mask):
    from train import decoded as dec
    return dec(crf, logits, padding_mask)


def _speaker_kw(model, batch, device):
    from train import _speaker_kw as kw
    return kw(model, batch, device)


def test(model, dl_test, device):
    """-> (accuracy, weighted_f1) over the loader, per-batch scores averaged unweighted.
    With ``model.streaming`` (runtime.streaming) every batch goes through ``DialogueStream.run`` - column by column, one new utterance per
    dialogue and step, or ``model.stream_chunk`` (runtime.stream_chunk) columns per chunk call - and its logits are scored as the batched
    pass's are (on the host).
    With ``model.device_metrics`` (runtime.device_metrics) every batch is scored on the device (``M2FNet.eval_step``) and the host
    reads the record once; ``model.test_scores`` then holds the pass's ``DeviceScores`` (confusion matrix, per-class report).
    With ``model.attention_maps_out`` (runtime.attention_maps) the batched passes also write every dialogue's attention maps."""
    model.eval()
    maps = _MapCollector(model)
    if getattr(model, "streaming", False):
        scores = BatchScores()
        with torch.inference_mode():
            for batch in tqdm(dl_test, total=len(dl_test)):
                text, audio, emotion, padding_mask = move_batch(batch, device, text_encoder=getattr(model, "text_encoder", None),
                                                               audio_encoder=getattr(model, "audio_encoder", None))
                stream = _stream_for(model, *padding_mask.shape)
                scores.update(stream.run(text, audio, padding_mask, **_speaker_kw(model, batch, device)), emotion)
        return scores.result()
    if getattr(model, "device_metrics", False):
        from mer_amd.metrics import DeviceScores
        scores = DeviceScores(model.m2f_config.cls_out, device)
        gamma = getattr(model, "focal_gamma", None)            # (solver.loss_fn: Focal; set by main())
        focal = {} if gamma is None else {"focal_gamma": gamma}
        if getattr(model, "crf", None) is not None:        # (the CRF loss and the Viterbi path)
            focal = {"label_smoothing": 0.0, "crf": model.crf}
        from train import AuxAccuracy
        aux_acc = AuxAccuracy(model)
        with torch.inference_mode():
            for batch in tqdm(dl_test, total=len(dl_test)):
                text, audio, emotion, padding_mask = move_batch(batch, device, text_encoder=getattr(model, "text_encoder", None),
                                                               audio_encoder=getattr(model, "audio_encoder", None))
                model.eval_step(text, audio, padding_mask, emotion, scores, **_speaker_kw(model, batch, device), **focal)
                aux_acc.update(model, batch, device)
                maps.add(padding_mask)
        model.test_scores = scores
        maps.write()
        if aux_acc.result() is not None:
            model.aux_test_accuracy = aux_acc.result()
            print(f"Aux_accuracy=[{aux_acc.result() * 100:.3f}%]")
        return scores.result()
    scores = BatchScores()
    from train import AuxAccuracy
    aux_acc = AuxAccuracy(model)                              # (runtime.aux_head: the head's accuracy beside the emotion scores)
    with torch.inference_mode():
        for batch in tqdm(dl_test, total=len(dl_test)):
            text, audio, emotion, padding_mask = move_batch(batch, device, text_encoder=getattr(model, "text_encoder", None),
                                                           audio_encoder=getattr(model, "audio_encoder", None))
            logits = model(text, audio, padding_mask, **_speaker_kw(model, batch, device))
            scores.update(decoded(getattr(model, "crf", None), logits, padding_mask), emotion)
            aux_acc.update(model, batch, device)
            maps.add(padding_mask)
    maps.write()
    if aux_acc.result() is not None:
        model.aux_test_accuracy = aux_acc.result()
        print(f"Aux_accuracy=[{aux_acc.result() * 100:.3f}%]")
    return scores.result()


def print_class_report(report):
    """Per-class precision / recall / F1 / support of the pass (DeviceScores.report())."""
    print(f"{'class':>5} {'precision':>9} {'recall':>9} {'f1':>9} {'support':>8}")
    for c, (p, r, f, s) in enumerate(zip(report["precision"], report["recall"], report["f1"], report["support"])):
        print(f"{c:>5} {p * 100:>8.3f}% {r * 100:>8.3f}% {f * 100:>8.3f}% {s:>8}")


def build_model(config, device):
    """The model as train.py built it (train.build_model): runtime.precision, runtime.context, runtime.position_bias and
    runtime.speaker_heads, so a model trained under a context band, a position bias or speaker heads is tested under it."""
    from train import build_model as build
    return build(config, device)


def main(config=None):
    config = get_config()
    from train import context_settings, position_bias_settings, speaker_heads_settings
    context_settings(config)                               # (refusal before the GPU is touched)
    position_bias_settings(config)
    spk_on = speaker_heads_settings(config) is not None    # (the test table then yields "speaker" ids)
    from train import aux_head_settings
    aux_on = aux_head_settings(config)                     # (the test table then yields the second label; refuses the device batcher)
    streaming = streaming_settings(config)
    stream_chunk = stream_chunk_settings(config)
    stream_pages = stream_pages_settings(config)
    attention_maps = attention_maps_settings(config)
    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    print(f"Using device {device}...")
    runtime_cfg = config.get("runtime", {}) or {}
    if runtime_cfg.get("device_batcher", False):
        loader = DeviceLoader(Dataset(mode="test"), device=device, **config.test.data_loader)
    else:
        ds_kw = dict(({"speakers": True} if spk_on else {}), **({aux_on["labels"]: True} if aux_on is not None else {}))
        loader = torch.utils.data.DataLoader(Dataset(mode="test", **ds_kw), collate_fn=collate_fn, **config.test.data_loader)
    model = build_model(config, device)
    model.device_metrics = bool(runtime_cfg.get("device_metrics", False))
    model.streaming = streaming
    model.stream_chunk = stream_chunk
    model.stream_pages = stream_pages
    model.attention_maps_out = attention_maps
    from train import attach_crf, build_crf, crf_settings, ema_settings, focal_gamma_setting
    # (solver.loss_fn: CRF - the block comes from the checkpoint's 'crf_state_dict'; batched passes decode with Viterbi)
    attach_crf(model, build_crf(dict(crf_settings(config), init="zeros", trainable=False), None, device) if config.solver.loss_fn == "CRF" else None)
    # (solver.loss_fn: Focal - the device record's loss is the criterion that trained, with runtime.focal_gamma; accuracy and F1 do not depend on it)
    model.focal_gamma = focal_gamma_setting(config) if config.solver.loss_fn == "Focal" else None
    ema = ema_settings(config)
    # (runtime.aux_head - the head comes from the checkpoint's 'aux_head_state_dict'; the pass also prints its accuracy)
    from train import attach_aux_head
    attach_aux_head(model, aux_on, config.model.CLASSIFIER.hidden_size, device, with_optimizer=False)
    load_model_weights(model, config.checkpoint.load_path, device, averaged=ema is not None and ema[2])
    print("Testing...")
    accuracy, weighted_f1 = test(model, loader, device)
    print(f"Accuracy=[{accuracy * 100:.3f}%] Weighted_F1=[{weighted_f1 * 100:.3f}%]")
    if model.device_metrics:
        print_class_report(model.test_scores.report())
    print("Testing complete")


if __name__ == "__main__":
    main()
