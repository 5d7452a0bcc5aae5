"""Checkpoint surgery between the pre-training tasks and AffWild2VA -- stage 3 of the reference's workflow, the behaviour of its two
scripts process/export_pretrained_ckpts.py and process/merge_av_checkpoints.py as importable functions:

  export_pretrained_video(sd)   a VoxCeleb2_1k state dict (models/vox2_model.py, `--backbone v2p`) -> the keys of a `v2p_split` tower
                                with split_layer = 3: the classifier `visual.fc.*` is dropped, stem layers `visual.v2p.<i>.*` with
                                i < 12 (conv1-conv3) become `visual.shared.<i>.*`, layers i >= 12 (conv4, conv5) initialise BOTH private
                                towers, `visual.v_private.<i-12>.*` and `visual.a_private.<i-12>.*` (the same tensor under both keys).
  merge_av(audio_sd, video_sd)  an AudioSet state dict (models/audioset_model.py) and a video state dict (the export above, or a trained
                                visual AffWild2VA) -> one audiovisual state dict: the classifier heads `audio.fc.*`,
                                `visual.gru_v.fc.*` and `visual.gru_a.fc.*` are dropped, everything else is kept, audio first.

Both take a state dict or a checkpoint ({'state_dict': ...}) and return {'state_dict': OrderedDict}, which
`AffWild2VA(modality='audiovisual', backbone='v2p_split', split_layer=3).load_state_dict(..., strict=False)` takes without unexpected keys.

    python -m m3t.checkpoints export vox2.ckpt video_checkpoint.pt
    python -m m3t.checkpoints merge audioset.ckpt video_checkpoint.pt fused_av.pt
"""
import sys
from collections import OrderedDict

SPLIT_AT = 12      # modules of the VGG-M stem up to conv3 (4 + 4 + 4: convolution, normalisation, ReLU, pooling each)


def _sd(ckpt):
    return ckpt['state_dict'] if 'state_dict' in ckpt else ckpt


def export_pretrained_video(state_dict):
    out = OrderedDict()
    for k, w in _sd(state_dict).items():
        if k.startswith('visual.fc'):
            continue
        parts = k.split('.')
        if parts[:2] != ['visual', 'v2p']:
            raise KeyError("export_pretrained_video: not a VoxCeleb2_1k (--backbone v2p) key: %s" % k)
        layer, rest = int(parts[2]), '.'.join(parts[3:])
        if layer < SPLIT_AT:
            out['visual.shared.%d.%s' % (layer, rest)] = w
        else:
            out['visual.v_private.%d.%s' % (layer - SPLIT_AT, rest)] = w
            out['visual.a_private.%d.%s' % (layer - SPLIT_AT, rest)] = w
    return OrderedDict(state_dict=out)


def merge_av(audio_sd, video_sd):
    out = OrderedDict()
    for k, w in _sd(audio_sd).items():
        if not k.startswith('audio.fc'):
            out[k] = w
    for k, w in _sd(video_sd).items():
        if not (k.startswith('visual.gru_a.fc') or k.startswith('visual.gru_v.fc')):
            out[k] = w
    return OrderedDict(state_dict=out)


def main(argv):
    import torch
    if len(argv) == 3 and argv[0] == 'export':
        torch.save(export_pretrained_video(torch.load(argv[1], map_location='cpu')), argv[2])
    elif len(argv) == 4 and argv[0] == 'merge':
        torch.save(merge_av(torch.load(argv[1], map_location='cpu'), torch.load(argv[2], map_location='cpu')), argv[3])
    else:
        print(__doc__.split('\n\n')[-1], file=sys.stderr)
        return 2
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
