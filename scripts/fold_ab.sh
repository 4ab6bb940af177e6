for f in 0 1; do
  line=$(ARP_LN_FOLD=$f python bench.py --full --mode bf16 --no-secondary --cpu-seconds 0 --parity-frames 8 --timed-only --steps 30 2>/dev/null | tail -1)
  python -c "import json, sys; d = json.loads(sys.argv[1]); print('bf16 ARP_LN_FOLD=$f', round(d['value']), round(d['ms_per_step'], 3), d['parity']['max_cosine_err_vs_oracle'])" "$line"
done
