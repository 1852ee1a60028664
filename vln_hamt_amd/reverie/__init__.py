"""Mirror of the reference package ``finetune_src/reverie`` (vlnbert_navref, model_navref): REVERIE's object-grounding model."""
