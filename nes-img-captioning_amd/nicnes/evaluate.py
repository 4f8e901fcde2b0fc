"""python -m nicnes.evaluate -- captions and metrics of a trained theta on a split: the counterpart of the reference's
eval_on_test.py (CaptPolicy.accuracy_on -> eval_split, captioning/eval_utils.py:110-180), on the GPU.

    python -m nicnes.evaluate --exp experiments/mscoco_nes.json --model logs/.../0_0_elite.pth --split test \\
        --num -1 --out test_eval.json

Writes {'stats': {'Bleu_1'..'Bleu_4', 'ROUGE_L', 'CIDEr'}, 'predictions': [{'image_id', 'caption'}]} as JSON. The
metrics are computed on the split's label rows (word ids, captions cut to seq_length words, rare words as UNK), not
on PTB-tokenised raw annotations; METEOR and SPICE (java) are not computed (nicnes.validation). --beam_size K (1..8)
decodes with the engine's beam search (sum of log-probs, no length normalisation) instead of greedily. --xent adds
the teacher-forced validation loss and perplexity of theta on the split's label rows to the stats ('val_loss',
'val_perplexity') and prints them.
"""
import argparse
import importlib
import json
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--exp', required=True, help='experiment JSON (caption_options name the data)')
    ap.add_argument('--model', required=True, help='theta as a state_dict .pth (a snapshot\'s current or best model)')
    ap.add_argument('--split', default='test', choices=['val', 'test'])
    ap.add_argument('--num', type=int, default=None, help='images (default config.num_val_items; -1: the whole split)')
    ap.add_argument('--out', required=True)
    ap.add_argument('--incl_gts', action='store_true', help='add the reference captions to every prediction')
    ap.add_argument('--beam_size', type=int, default=None, choices=range(1, 9), metavar='K',
                    help='beam width 1..8 of the decode (default: greedy)')
    ap.add_argument('--xent', action='store_true',
                    help='add the teacher-forced cross-entropy (val_loss, val_perplexity) of the label rows')
    ap.add_argument('--data_root', default='.', help="directory the caption_options paths are relative to")
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--engine_factory', default=None, help='module:function(spec, args) -> engine (default: an Engine)')
    return ap.parse_args(argv)


def default_engine(spec, args):
    import nicnes
    return nicnes.Engine(device=args.device, **spec.engine_kwargs(max_members=1, noise_len=1 << 23))


def main(argv=None):
    args = parse_args(argv)
    from . import config as C
    from . import data
    from .nes import EnginePolicy
    from .validation import Validator
    exp = C.load_experiment(args.exp)
    loader = data.loader_from_caption_options(exp, int(exp['config'].get('batch_size') or 1), root=args.data_root)
    spec = C.ExperimentSpec(exp, vocab_size=loader.vocab_size, seq_length=loader.seq_length)
    if args.engine_factory:
        mod, fn = args.engine_factory.split(':')
        engine = getattr(importlib.import_module(mod), fn)(spec, args)
    else:
        engine = default_engine(spec, args)
    EnginePolicy(engine).set_model(args.model)
    num = args.num if args.num is not None else spec.config.num_val_items
    extra = {'xent': True} if args.xent else {}
    validator = Validator(engine, loader, args.split, 5000 if num is None else int(num), beam_size=args.beam_size, **extra)
    stats, predictions = validator.eval_split(incl_gts=args.incl_gts)
    if args.xent:
        print('loss %.6f perplexity %.4f' % (stats['val_loss'], stats['val_perplexity']))
    with open(args.out, 'w') as f:
        json.dump({'stats': stats, 'predictions': predictions}, f)
    validator.close()
    if hasattr(engine, 'close'):
        engine.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
